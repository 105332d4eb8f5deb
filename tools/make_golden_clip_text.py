"""g19: the CLIP text tower fixture (tests/golden/g19_clip_text_tiny.npz), written by the installed transformers on the CPU.

  python tools/make_golden_clip_text.py

A tiny random-init CLIPTextModelWithProjection (eager attention, fp32; the weights hold bf16-representable values and are stored as
their 16-bit patterns) on eight right-padded rows of lengths 3, 4, 9, 16, 17, 40, 76, 77 (pad id = eos id = 95).  The hidden states are
stored at the valid positions only, in packed order; text_embeds and the unit features are stored under both pooling rules of
hf:clip/modeling_clip.py:561-581 from the same weights - config eos_token_id = 2 (the first position of the row's largest id) and
eos_token_id = 95 (the first position of that id).  Two rows tell the rules from "the last valid token": the 17-token row holds a
second 95 at position 5 (both rules pool there), and the unpadded 77-token row holds no 95 at all, so the first rule pools its largest
id (94, at position 40) and the second, as argmax over an all-false row does, position 0."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "g19_clip_text_tiny.npz"
TINY = dict(vocab_size=96, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
            projection_dim=32)
LENGTHS = [3, 4, 9, 16, 17, 40, 76, 77]
BOS, EOS = 1, 95             # pad id = eos id, as the public CLIP tokenizers have it


def rows():
    rng = np.random.default_rng(19)
    S = max(LENGTHS)
    ids = np.full((len(LENGTHS), S), EOS, dtype=np.int64)
    mask = np.zeros((len(LENGTHS), S), dtype=np.int64)
    for i, n in enumerate(LENGTHS):
        ids[i, :n] = rng.integers(3, 94, n)                 # ordinary tokens: 3 .. 93
        ids[i, 0] = BOS
        ids[i, n - 1] = EOS
        mask[i, :n] = 1
    ids[LENGTHS.index(17), 5] = EOS
    last = LENGTHS.index(77)
    ids[last, 76] = 60
    ids[last, 40] = 94
    return ids, mask


def main():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    torch.manual_seed(19)
    cfg = CLIPTextConfig(**TINY, pad_token_id=EOS, bos_token_id=BOS, eos_token_id=2)
    cfg._attn_implementation = "eager"
    model = CLIPTextModelWithProjection(cfg).eval()
    with torch.no_grad():                                    # HF's init leaves biases 0 and norms 1: move them so every term is exercised
        for k, p in model.named_parameters():
            if k.endswith(".bias"):
                p.normal_(0, 0.02)
            elif "layer_norm" in k:
                p.normal_(1.0, 0.1)
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    ids, mask = rows()
    arrays = {"wbf16::" + k: v.detach().to(torch.bfloat16).view(torch.int16).numpy() for k, v in model.state_dict().items()
              if not k.endswith("position_ids")}
    arrays["cfg_keys"] = np.array(list(TINY) + ["layer_norm_eps"])
    arrays["cfg_vals"] = np.array([float(v) for v in TINY.values()] + [float(cfg.layer_norm_eps)])
    arrays["hidden_act"] = np.array(cfg.hidden_act)
    arrays["input_ids"] = ids.astype(np.int16)
    arrays["attention_mask"] = mask.astype(np.int8)
    arrays["lengths"] = np.array(LENGTHS)
    valid = torch.from_numpy(mask) != 0
    for eos in (2, EOS):
        model.text_model.eos_token_id = eos                  # what CLIPTextTransformer.forward reads (set from config.eos_token_id)
        model.config.eos_token_id = eos
        with torch.no_grad():
            out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), output_hidden_states=True)
        if eos == 2:
            for i, h in enumerate(out.hidden_states):
                arrays[f"hidden_{i}"] = h[valid].numpy()
        arrays[f"eos{eos}::text_embeds"] = out.text_embeds.numpy()
        arrays[f"eos{eos}::features"] = (out.text_embeds / out.text_embeds.norm(dim=-1, keepdim=True)).numpy()
    d = np.abs(arrays["eos2::text_embeds"] - arrays[f"eos{EOS}::text_embeds"]).max(1)
    print("rows whose two pooling rules differ:", np.nonzero(d > 0)[0].tolist())
    np.savez_compressed(OUT, **arrays)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
