"""CPU restatements that the retrieval tests judge against (oracle/ is frozen, so they live beside the tests): the exact search in
float64 and the CLIP vision tower with projection (hf:clip/modeling_clip.py CLIPVisionModelWithProjection) in plain torch ops."""
from __future__ import annotations

import numpy as np
import torch


def topk_ip_ref(q, x, k):
    """float64 scores, stable argsort: rows sorted by (score descending, index ascending).  -> (idx (Q, k) int64, score (Q, k) fp32)."""
    q, x = np.asarray(q), np.asarray(x)
    s = q.astype(np.float64) @ x.astype(np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k].astype(np.int64)
    return order, np.take_along_axis(s, order, axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CLIP image tower
def _act(x, name):
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)                   # hf:activations.py QuickGELUActivation
    if name == "gelu":
        return torch.nn.functional.gelu(x)
    raise ValueError(name)


def clip_vision_forward(sd, arch, pixel_values, dtype=torch.float32, device="cpu"):
    """hf:clip/modeling_clip.py CLIPVisionModelWithProjection.forward (eager attention) in plain torch ops, every op in `dtype`.
    sd: state dict with the HF key names; arch: anything with the CLIPVisionConfig fields + projection_dim.
    -> dict(hidden_states=[embedding output, layer outputs...], pooled, image_embeds, features (unit rows, fp32))."""
    F = torch.nn.functional
    g = lambda k: sd[k].to(device=device, dtype=dtype)
    E, nh, eps = arch.hidden_size, arch.num_attention_heads, arch.layer_norm_eps
    hd = E // nh
    vp = "vision_model."
    pix = pixel_values.to(device=device, dtype=dtype)
    n = pix.shape[0]
    with torch.no_grad():
        patches = F.conv2d(pix, g(vp + "embeddings.patch_embedding.weight"), stride=arch.patch_size).flatten(2).transpose(1, 2)
        x = torch.cat([g(vp + "embeddings.class_embedding").expand(n, 1, E), patches], dim=1) + g(vp + "embeddings.position_embedding.weight")
        x = F.layer_norm(x, (E,), g(vp + "pre_layrnorm.weight"), g(vp + "pre_layrnorm.bias"), eps)
        T = x.shape[1]
        hidden = [x]
        for i in range(arch.num_hidden_layers):
            p = f"{vp}encoder.layers.{i}."
            lin = lambda t, name: F.linear(t, g(p + name + ".weight"), g(p + name + ".bias"))
            y = F.layer_norm(x, (E,), g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), eps)
            q, k, v = (lin(y, f"self_attn.{m}_proj").view(n, T, nh, hd).transpose(1, 2) for m in ("q", "k", "v"))
            w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5, dim=-1, dtype=torch.float32).to(dtype)
            o = torch.matmul(w, v).transpose(1, 2).reshape(n, T, E)
            x = x + lin(o, "self_attn.out_proj")
            y = F.layer_norm(x, (E,), g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), eps)
            x = x + lin(_act(lin(y, "mlp.fc1"), arch.hidden_act), "mlp.fc2")
            hidden.append(x)
        pooled = F.layer_norm(x[:, 0, :], (E,), g(vp + "post_layernorm.weight"), g(vp + "post_layernorm.bias"), eps)
        embeds = F.linear(pooled, g("visual_projection.weight"))
        feats = embeds.float()
        feats = feats / feats.norm(dim=-1, keepdim=True)
    return dict(hidden_states=hidden, pooled=pooled, image_embeds=embeds, features=feats)


# ------------------------------------------------------------------------------------------------ CLIP image pre-processing
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)               # hf:utils/constants.py OPENAI_CLIP_MEAN / _STD
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_resize_crop_u8(img, size):
    """hf CLIPImageProcessor up to the rescale: RGB, shortest edge -> `size` (bicubic, the long edge truncated with int()), centre crop
    size x size.  PIL image -> (size, size, 3) uint8."""
    from PIL import Image
    img = img.convert("RGB")
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    img = img.resize((nw, nh), resample=Image.BICUBIC)
    top, left = (nh - size) // 2, (nw - size) // 2
    return np.asarray(img.crop((left, top, left + size, top + size)), dtype=np.uint8)


def clip_preprocess_ref(images, size):
    """list of PIL images -> (n, 3, size, size) fp32: the host restatement of CLIPImageProcessor."""
    u8 = np.stack([clip_resize_crop_u8(im, size) for im in images])
    x = (u8.astype(np.float64) * (1 / 255)).astype(np.float32)            # hf:image_transforms.py rescale: float64 product, one rounding
    x = (x - np.asarray(CLIP_MEAN, dtype=np.float32)) / np.asarray(CLIP_STD, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ the g18 fixture
def load_g18(npz):
    """tests/golden/g18_clip_tiny.npz (tools/make_golden_clip.py) -> (ClipVisionArch, fp32 state dict, pixel_values fp32)."""
    from licv.config import ClipVisionArch
    unbf = lambda a: torch.from_numpy(a.copy()).view(torch.bfloat16).float()
    cfg = {k: float(v) for k, v in zip(npz["cfg_keys"].tolist(), npz["cfg_vals"].tolist())}
    kw = {k: (v if k == "layer_norm_eps" else int(v)) for k, v in cfg.items()}
    arch = ClipVisionArch(hidden_act=str(npz["hidden_act"]), **kw)
    sd = {k[len("wbf16::"):]: unbf(npz[k]) for k in npz.files if k.startswith("wbf16::") and not k.endswith("position_ids")}
    return arch, sd, unbf(npz["pixel_values_bf16"])
