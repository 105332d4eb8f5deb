"""The CLIP image tower with projection (hf:clip/modeling_clip.py CLIPVisionModelWithProjection) on the library's kernels: what the
reference's retriever encodes every index and test image with (ref:icv_src/utils/mm_topk_retriver.py, mode "i2i").

bf16 weights and activations like both LMM engines; the features leave as fp32 unit rows (what the reference hands to faiss).  The
tower is the Idefics vision tower's architecture family and runs on the same ops (im2col + GEMM patch embedding, fused cls + position +
pre_layrnorm, LayerNorm, unmasked attention, GEMMs with bias / residual epilogues); new are QuickGELU, the class-token pick (a strided
LayerNorm: row 0 of every T) and the row normalisation."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Tuple

import torch

from . import ops
from .config import ClipVisionArch
from .idefics_engine import _bf, _pad_cols, _VitLayer


def clip_vision_state(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The tower's tensors under the key names of CLIPVisionModelWithProjection (`vision_model.*`, `visual_projection.weight`): those
    are also the names inside a full CLIPModel checkpoint, whose `text_model.*`, `text_projection.weight` and `logit_scale` are dropped."""
    out = {k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    if "visual_projection.weight" not in out or "vision_model.embeddings.class_embedding" not in out:
        raise KeyError("state dict holds no CLIP vision tower (vision_model.*, visual_projection.weight)")
    return out


def load_clip_vision(path) -> Tuple[ClipVisionArch, Dict[str, torch.Tensor]]:
    """(arch, state dict) from a local directory with config.json + *.safetensors shards."""
    from .checkpoint import read_config_json, read_safetensors_dir
    path = Path(path)
    sd = read_safetensors_dir(path)
    return ClipVisionArch.from_hf(read_config_json(path)), clip_vision_state(sd)


class ClipVisionEngine:
    def __init__(self, arch: ClipVisionArch, state_dict: Dict[str, torch.Tensor], device="cuda"):
        a, dev = arch, torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ClipVisionEngine runs on the GPU only (liblicv_hip has no CPU fallback)")
        sd = clip_vision_state(state_dict)
        self.arch, self.device = a, dev
        g = lambda k: _bf(sd[k], dev)
        vp = "vision_model."
        self.patch_ld = (3 * a.patch_size * a.patch_size + 63) // 64 * 64
        self.patch_w = _pad_cols(g(vp + "embeddings.patch_embedding.weight").flatten(1), self.patch_ld)
        self.cls = g(vp + "embeddings.class_embedding")
        self.pos = g(vp + "embeddings.position_embedding.weight")
        assert self.pos.shape == (a.tokens, a.hidden_size), f"position table {tuple(self.pos.shape)} does not match the config"
        self.pre_ln_w, self.pre_ln_b = g(vp + "pre_layrnorm.weight"), g(vp + "pre_layrnorm.bias")
        self.layers = []
        for i in range(a.num_hidden_layers):
            p = f"{vp}encoder.layers.{i}."
            cat = lambda suf: torch.cat([g(p + f"self_attn.{n}_proj.{suf}") for n in ("q", "k", "v")]).contiguous()
            self.layers.append(_VitLayer(g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), cat("weight"), cat("bias"),
                                         g(p + "self_attn.out_proj.weight"), g(p + "self_attn.out_proj.bias"),
                                         g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"),
                                         g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias"), g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")))
        self.post_ln_w, self.post_ln_b = g(vp + "post_layernorm.weight"), g(vp + "post_layernorm.bias")
        self.proj_w = g("visual_projection.weight")
        assert self.proj_w.shape == (a.projection_dim, a.hidden_size)

    @torch.no_grad()
    def image_embeds(self, pixel_values: torch.Tensor, hidden_states=None) -> torch.Tensor:
        """pixel_values (n, 3, S, S) -> the un-normalised image_embeds (n, projection_dim) bf16, one pass for the whole batch.
        `hidden_states`: a list that receives HF's output_hidden_states (the embedding output and every layer's), for tests."""
        a = self.arch
        pix = pixel_values.to(device=self.device, dtype=torch.bfloat16).contiguous()
        assert pix.dim() == 4 and pix.shape[1] == 3 and pix.shape[2] == pix.shape[3] == a.image_size, \
            f"pixel_values {tuple(pix.shape)}: (n, 3, {a.image_size}, {a.image_size}) expected"
        n, E, T, nh, hd = pix.shape[0], a.hidden_size, a.tokens, a.num_attention_heads, a.head_dim
        cols = ops.im2col_patches(pix, a.patch_size, self.patch_ld)
        patches = ops.linear(cols, self.patch_w)
        x = ops.vit_embed_ln(patches, self.cls, self.pos, self.pre_ln_w, self.pre_ln_b, n, T - 1, a.layer_norm_eps).view(n * T, E)
        del cols, patches
        if hidden_states is not None:
            hidden_states.append(x.view(n, T, E).clone())
        for L in self.layers:
            y = ops.layernorm(x, L.ln1_w, L.ln1_b, a.layer_norm_eps)
            qkv = ops.linear(y, L.qkv_w, bias=L.qkv_b)
            o = ops.attention(qkv, qkv.view(-1)[E:], qkv.view(-1)[2 * E:], n, T, T, nh, nh, hd,
                              T * 3 * E, 3 * E, T * 3 * E, 3 * E, hd ** -0.5, 0)
            del qkv
            ops.linear(o.view(n * T, E), L.out_w, bias=L.out_b, residual=x, out=x)
            y = ops.layernorm(x, L.ln2_w, L.ln2_b, a.layer_norm_eps)
            if a.hidden_act == "quick_gelu":
                y = ops.quick_gelu_(ops.linear(y, L.fc1_w, bias=L.fc1_b))
            else:
                y = ops.linear(y, L.fc1_w, bias=L.fc1_b, act="gelu")
            ops.linear(y, L.fc2_w, bias=L.fc2_b, residual=x, out=x)
            del y, o
            if hidden_states is not None:
                hidden_states.append(x.view(n, T, E).clone())
        # pooled = post_layernorm(last_hidden_state[:, 0]): a LayerNorm over row 0 of every T rows
        pooled = torch.empty((n, E), dtype=torch.bfloat16, device=self.device)
        ops.layernorm(x, self.post_ln_w, self.post_ln_b, a.layer_norm_eps, out=pooled, rows=n, dim=E, ld_x=T * E, ld_out=E)
        return ops.linear(pooled, self.proj_w)

    @torch.no_grad()
    def encode(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values (n, 3, S, S) -> (n, projection_dim) fp32 unit rows on the device."""
        return ops.l2_normalize_rows(self.image_embeds(pixel_values).contiguous())
