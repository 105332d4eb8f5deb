"""CPU restatement of the CLIP text tower with projection (hf:clip/modeling_clip.py CLIPTextModelWithProjection, eager attention) in
plain torch ops on the PADDED batch, as transformers runs it; the text-tower tests judge the packed GPU engine against it.  Beside the
tests because oracle/ is frozen (as tests/clip_ref.py)."""
from __future__ import annotations

import numpy as np
import torch

from clip_ref import _act


def pooled_positions(input_ids, eos_token_id):
    """hf:clip/modeling_clip.py:561-581 on the padded ids: eos_token_id == 2 -> argmax of the ids, else the first eos_token_id."""
    ids = input_ids.to(torch.int)
    return ids.argmax(dim=-1) if eos_token_id == 2 else (ids == eos_token_id).int().argmax(dim=-1)


def clip_text_forward(sd, arch, input_ids, attention_mask=None, dtype=torch.float32, device="cpu"):
    """sd: state dict with the HF key names; arch: anything with the CLIPTextConfig fields + projection_dim; input_ids, attention_mask
    (n, S) right- or un-padded.  Every op in `dtype`.
    -> dict(hidden_states=[embedding output, layer outputs...] (n, S, E), pooled, text_embeds, features (unit rows, fp32))."""
    F = torch.nn.functional
    g = lambda k: sd[k].to(device=device, dtype=dtype)
    E, nh, eps = arch.hidden_size, arch.num_attention_heads, arch.layer_norm_eps
    hd = E // nh
    tp = "text_model."
    ids = torch.as_tensor(input_ids).to(device=device, dtype=torch.int64)
    n, S = ids.shape
    mask = torch.ones_like(ids) if attention_mask is None else torch.as_tensor(attention_mask).to(device=device)
    allowed = torch.tril(torch.ones(S, S, dtype=torch.bool, device=device))[None, None] & (mask != 0)[:, None, None, :]
    bias = torch.zeros((n, 1, S, S), dtype=dtype, device=device).masked_fill(~allowed, torch.finfo(dtype).min)
    with torch.no_grad():
        x = F.embedding(ids, g(tp + "embeddings.token_embedding.weight")) + g(tp + "embeddings.position_embedding.weight")[:S]
        hidden = [x]
        for i in range(arch.num_hidden_layers):
            p = f"{tp}encoder.layers.{i}."
            lin = lambda t, name: F.linear(t, g(p + name + ".weight"), g(p + name + ".bias"))
            y = F.layer_norm(x, (E,), g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), eps)
            q, k, v = (lin(y, f"self_attn.{m}_proj").view(n, S, nh, hd).transpose(1, 2) for m in ("q", "k", "v"))
            w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5 + bias, dim=-1, dtype=torch.float32).to(dtype)
            o = torch.matmul(w, v).transpose(1, 2).reshape(n, S, E)
            x = x + lin(o, "self_attn.out_proj")
            y = F.layer_norm(x, (E,), g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), eps)
            x = x + lin(_act(lin(y, "mlp.fc1"), arch.hidden_act), "mlp.fc2")
            hidden.append(x)
        last = F.layer_norm(x, (E,), g(tp + "final_layer_norm.weight"), g(tp + "final_layer_norm.bias"), eps)
        pooled = last[torch.arange(n, device=device), pooled_positions(ids, arch.eos_token_id)]
        embeds = F.linear(pooled, g("text_projection.weight"))
        feats = embeds.float()
        feats = feats / feats.norm(dim=-1, keepdim=True)
    return dict(hidden_states=hidden, pooled=pooled, text_embeds=embeds, features=feats)


def valid_rows(t, attention_mask):
    """(n, S, E) -> the (total, E) rows at the mask's valid positions, row-major: the packed order."""
    return t[torch.as_tensor(attention_mask) != 0]


# ------------------------------------------------------------------------------------------------ the g19 fixture
def load_g19(npz, eos_token_id):
    """tests/golden/g19_clip_text_tiny.npz (tools/make_golden_clip_text.py) under one of its two pooling rules (config eos_token_id 2 or
    95) -> (ClipTextArch, fp32 state dict, input_ids (n, S) int64, attention_mask (n, S) int64, recorded outputs: dict with hidden_<i>
    (total, E) at the valid positions, text_embeds, features)."""
    from licv.config import ClipTextArch
    unbf = lambda a: torch.from_numpy(a.copy()).view(torch.bfloat16).float()
    cfg = {k: float(v) for k, v in zip(npz["cfg_keys"].tolist(), npz["cfg_vals"].tolist())}
    kw = {k: (v if k == "layer_norm_eps" else int(v)) for k, v in cfg.items()}
    arch = ClipTextArch(hidden_act=str(npz["hidden_act"]), eos_token_id=int(eos_token_id), **kw)
    sd = {k[len("wbf16::"):]: unbf(npz[k]) for k in npz.files if k.startswith("wbf16::") and not k.endswith("position_ids")}
    tag = f"eos{int(eos_token_id)}::"
    out = {k[len(tag):]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(tag)}
    for k in npz.files:                                        # the hidden states do not depend on the pooling rule: stored once
        if k.startswith("hidden_") and k != "hidden_act":
            out[k] = torch.from_numpy(npz[k])
    return arch, sd, torch.from_numpy(npz["input_ids"].astype(np.int64)), torch.from_numpy(npz["attention_mask"].astype(np.int64)), out
