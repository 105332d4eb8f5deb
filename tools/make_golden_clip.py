"""g18: the CLIP image tower fixture (tests/golden/g18_clip_tiny.npz), written by the installed transformers on the CPU.

  python tools/make_golden_clip.py

A tiny random-init CLIPVisionModelWithProjection (eager attention, fp32): weights, pixel inputs, every hidden state, image_embeds and
the unit features (weights and pixels hold bf16-representable values and are stored as their 16-bit patterns); and the outputs of transformers' CLIP image processor (PIL backend) for a handful of synthetic PIL images of odd
sizes, stored with the images themselves so the tests need neither transformers nor an image file."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "g18_clip_tiny.npz"
TINY = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, image_size=64, patch_size=32,
            projection_dim=32)
# (width, height, mode): portrait, landscape, smaller than the target, grey-scale, square
IMAGES = [(100, 150, "RGB"), (165, 113, "RGB"), (40, 52, "RGB"), (130, 120, "L"), (64, 64, "RGB")]
PROC_SIZE = 64             # the tiny tower's image size: keeps the fixture small; the arithmetic does not depend on the size


def synthetic_image(w, h, mode, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = [127 + 90 * np.sin(xx / w * rng.uniform(2, 9) + yy / h * rng.uniform(2, 9) + rng.uniform(0, 6)) + rng.normal(0, 12, (h, w))
          for _ in range(1 if mode == "L" else 3)]
    a = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if mode == "L" else a, mode=mode)


def main():
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(18)
    cfg = CLIPVisionConfig(**TINY)
    cfg._attn_implementation = "eager"
    model = CLIPVisionModelWithProjection(cfg).eval()
    with torch.no_grad():                                    # HF's init leaves biases 0 and norms 1: move them so every term is exercised
        for k, p in model.named_parameters():
            if k.endswith(".bias"):
                p.normal_(0, 0.02)
            elif "layer_norm" in k or "layrnorm" in k or "layernorm" in k:
                p.normal_(1.0, 0.1)
        for p in model.parameters():                         # bf16-representable values: stored as 16-bit patterns (half the bytes), and the
            p.copy_(p.to(torch.bfloat16).float())            # bf16 engine loads them without a rounding of its own
    pix = torch.randn(4, 3, TINY["image_size"], TINY["image_size"]).to(torch.bfloat16).float()
    with torch.no_grad():
        out = model(pixel_values=pix, output_hidden_states=True)
    arrays = {"wbf16::" + k: v.detach().to(torch.bfloat16).view(torch.int16).numpy() for k, v in model.state_dict().items()}
    arrays["cfg_keys"] = np.array(list(TINY) + ["layer_norm_eps"])
    arrays["cfg_vals"] = np.array([float(v) for v in TINY.values()] + [float(cfg.layer_norm_eps)])
    arrays["hidden_act"] = np.array(cfg.hidden_act)
    arrays["pixel_values_bf16"] = pix.to(torch.bfloat16).view(torch.int16).numpy()
    for i, h in enumerate(out.hidden_states):
        arrays[f"hidden_{i}"] = h.numpy()
    arrays["image_embeds"] = out.image_embeds.numpy()
    f = out.image_embeds / out.image_embeds.norm(dim=-1, keepdim=True)
    arrays["features"] = f.numpy()

    proc = CLIPImageProcessor(size={"shortest_edge": PROC_SIZE}, crop_size={"height": PROC_SIZE, "width": PROC_SIZE})
    print("image processor:", type(proc).__name__)
    for i, (w, h, mode) in enumerate(IMAGES):
        im = synthetic_image(w, h, mode, 180 + i)
        arrays[f"img_{i}"] = np.asarray(im)
        arrays[f"proc_{i}"] = np.asarray(proc(images=im, return_tensors="np")["pixel_values"][0], dtype=np.float32)
    arrays["n_images"] = np.array(len(IMAGES))
    arrays["proc_size"] = np.array(PROC_SIZE)
    np.savez_compressed(OUT, **arrays)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
