"""The CLIP towers with projection (hf:clip/modeling_clip.py CLIPVisionModelWithProjection, CLIPTextModelWithProjection) on the
library's kernels: what the reference's retriever encodes every index and test image / text with
(ref:icv_src/utils/mm_topk_retriver.py encode_img, encode_text).

bf16 weights and activations like both LMM engines; the features leave as fp32 unit rows (what the reference hands to faiss).  The
tower is the Idefics vision tower's architecture family and runs on the same ops (im2col + GEMM patch embedding, fused cls + position +
pre_layrnorm, LayerNorm, unmasked attention, GEMMs with bias / residual epilogues); new are QuickGELU, the class-token pick (a strided
LayerNorm: row 0 of every T) and the row normalisation.

The text tower is causal, so it runs on the VALID tokens only, packed back to back (pack_text_batch): the token + position embedding on
packed ids, causal attention over the ragged batch (licv_attn_varlen_causal), the same GEMMs on `total` rows instead of n x S, and the
final LayerNorm on the end-of-text rows only.  That is exact, not an approximation: a right-padded row and the same row alone give the
same text_embeds in transformers.  There is no padded second path; ClipTextArch refuses what the packed kernels cannot serve."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import ops
from .blocks import bf16_on, dense_attend, encoder_layer_, load_encoder_layers, pad_cols
from .config import ClipTextArch, ClipVisionArch


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
        g = lambda k: bf16_on(sd[k], dev)
        vp = "vision_model."
        self.patch_ld = (3 * a.patch_size * a.patch_size + 63) // 64 * 64
        self.patch_w = pad_cols(g(vp + "embeddings.patch_embedding.weight").flatten(1), self.patch_ld)
        self.cls = g(vp + "embeddings.class_embedding")
        self.pos = g(vp + "embeddings.position_embedding.weight")
        assert self.pos.shape == (a.tokens, a.hidden_size), f"position table {tuple(self.pos.shape)} does not match the config"
        self.pre_ln_w, self.pre_ln_b = g(vp + "pre_layrnorm.weight"), g(vp + "pre_layrnorm.bias")
        self.layers = load_encoder_layers(g, vp + "encoder.layers.", a.num_hidden_layers)
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
        attend = dense_attend(n, T, nh, hd)
        for L in self.layers:
            encoder_layer_(x, L, a.layer_norm_eps, a.hidden_act, attend)
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


# ------------------------------------------------------------------------------------------------ text tower
def clip_text_state(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The tower's tensors under the key names of CLIPTextModelWithProjection (`text_model.*`, `text_projection.weight`): also the names
    inside a full CLIPModel checkpoint, whose vision tower and `logit_scale` are dropped."""
    out = {k: v for k, v in sd.items() if k.startswith("text_model.") or k == "text_projection.weight"}
    if "text_projection.weight" not in out or "text_model.embeddings.token_embedding.weight" not in out:
        raise KeyError("state dict holds no CLIP text tower (text_model.*, text_projection.weight)")
    return out


def load_clip_text(path) -> Tuple[ClipTextArch, Dict[str, torch.Tensor]]:
    """(arch, state dict) from a local directory with config.json + *.safetensors shards."""
    from .checkpoint import read_config_json, read_safetensors_dir
    path = Path(path)
    sd = read_safetensors_dir(path)
    return ClipTextArch.from_hf(read_config_json(path)), clip_text_state(sd)


class PackedText(NamedTuple):
    ids: torch.Tensor            # (total,) int64: the valid tokens of every row, back to back
    cu_seqlens: torch.Tensor     # (n + 1,) int32: row i = packed rows cu_seqlens[i] .. cu_seqlens[i + 1] - 1
    pool_rows: torch.Tensor      # (n,) int32: the PACKED row whose state is row i's pooled output
    positions: torch.Tensor      # (total,) int32: position of every packed token inside its row


def pack_text_batch(input_ids, attention_mask, arch: ClipTextArch) -> PackedText:
    """A right-padded tokenizer batch (input_ids, attention_mask: (n, S)) -> its valid tokens packed, all on the host.
    The pooled position follows hf:clip/modeling_clip.py:561-581 on the PADDED ids: with config eos_token_id == 2 the first position of
    the row's largest id, otherwise the first position of eos_token_id (position 0 when the row holds none, as argmax gives).
    ValueError: a mask that is not a non-empty prefix of ones, a length above max_position_embeddings, an id outside the vocabulary,
    a pooled position that falls into the padding (the padded tower would pool a padding state there)."""
    ids = torch.as_tensor(input_ids).cpu()
    if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8):
        raise ValueError(f"input_ids: an (n, S) integer tensor is expected, got {tuple(ids.shape)} {ids.dtype}")
    ids = ids.to(torch.int64)
    n, S = ids.shape
    mask = torch.ones((n, S), dtype=torch.int64) if attention_mask is None else torch.as_tensor(attention_mask).cpu().to(torch.int64)
    if mask.shape != ids.shape or n == 0 or S == 0:
        raise ValueError(f"attention_mask {tuple(mask.shape)} does not match input_ids {tuple(ids.shape)} (a non-empty batch is expected)")
    lens = mask.sum(1)
    valid = torch.arange(S)[None, :] < lens[:, None]
    if not torch.equal(mask != 0, valid) or not ((mask == 0) | (mask == 1)).all():
        bad = int(((mask != 0) != valid).any(1).nonzero()[0]) if not torch.equal(mask != 0, valid) else 0
        raise ValueError(f"attention_mask row {bad} is not a prefix of ones: only right-padded batches can be packed")
    if int(lens.min()) < 1:
        raise ValueError(f"attention_mask row {int(lens.argmin())} is empty")
    if int(lens.max()) > arch.max_position_embeddings:
        raise ValueError(f"row {int(lens.argmax())} holds {int(lens.max())} tokens, the tower has {arch.max_position_embeddings} positions "
                         f"(tokenize with truncation=True)")
    packed = ids[valid]
    if int(packed.min()) < 0 or int(packed.max()) >= arch.vocab_size:
        raise ValueError(f"token id {int(packed.max()) if int(packed.max()) >= arch.vocab_size else int(packed.min())} is outside the "
                         f"vocabulary [0, {arch.vocab_size})")
    pool = ids.argmax(dim=-1) if arch.eos_token_id == 2 else (ids == arch.eos_token_id).to(torch.int64).argmax(dim=-1)
    if (pool >= lens).any():
        bad = int((pool >= lens).nonzero()[0])
        raise ValueError(f"row {bad}: the pooled position {int(pool[bad])} (eos_token_id {arch.eos_token_id}) falls into the padding "
                         f"(the row holds {int(lens[bad])} tokens)")
    cu = torch.zeros(n + 1, dtype=torch.int64)
    cu[1:] = lens.cumsum(0)
    positions = (torch.arange(S)[None, :].expand(n, S))[valid]
    return PackedText(packed.contiguous(), cu.to(torch.int32), (cu[:-1] + pool).to(torch.int32), positions.to(torch.int32).contiguous())


class ClipTextEngine:
    def __init__(self, arch: ClipTextArch, state_dict: Dict[str, torch.Tensor], device="cuda"):
        a, dev = arch, torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ClipTextEngine runs on the GPU only (liblicv_hip has no CPU fallback)")
        sd = clip_text_state(state_dict)
        self.arch, self.device = a, dev
        g = lambda k: bf16_on(sd[k], dev)
        tp = "text_model."
        self.tok = g(tp + "embeddings.token_embedding.weight")
        self.pos = g(tp + "embeddings.position_embedding.weight")
        assert self.tok.shape == (a.vocab_size, a.hidden_size), f"token table {tuple(self.tok.shape)} does not match the config"
        assert self.pos.shape == (a.max_position_embeddings, a.hidden_size), f"position table {tuple(self.pos.shape)} does not match the config"
        self.layers = load_encoder_layers(g, tp + "encoder.layers.", a.num_hidden_layers)
        self.final_ln_w, self.final_ln_b = g(tp + "final_layer_norm.weight"), g(tp + "final_layer_norm.bias")
        self.proj_w = g("text_projection.weight")
        assert self.proj_w.shape == (a.projection_dim, a.hidden_size)

    @torch.no_grad()
    def text_embeds(self, input_ids, attention_mask=None, hidden_states: Optional[list] = None) -> torch.Tensor:
        """input_ids, attention_mask (n, S), right-padded -> the un-normalised text_embeds (n, projection_dim) bf16; one pass over the
        batch's valid tokens.  `hidden_states`: a list that receives the PACKED (total, hidden) states HF's output_hidden_states holds at
        the valid positions (the embedding output and every layer's), for tests."""
        a = self.arch
        pk = pack_text_batch(input_ids, attention_mask, a)
        E, nh, hd = a.hidden_size, a.num_attention_heads, a.head_dim
        cu_dev, rows_dev = pk.cu_seqlens.to(self.device), pk.pool_rows.to(self.device)
        x = ops.clip_text_embed(pk.ids.to(self.device), pk.positions.to(self.device), self.tok, self.pos)
        total = x.shape[0]
        if hidden_states is not None:
            hidden_states.append(x.clone())
        attend = lambda qkv: ops.attn_varlen_causal(qkv, pk.cu_seqlens, cu_dev, nh, hd, hd ** -0.5)
        for L in self.layers:
            encoder_layer_(x, L, a.layer_norm_eps, a.hidden_act, attend)
            if hidden_states is not None:
                hidden_states.append(x.clone())
        assert x.shape == (total, E)
        # pooled = final_layer_norm(last_hidden_state)[row, eos position]: the norm is row-wise, so only the pooled rows go through it
        pooled = ops.layernorm_rows(x, rows_dev, self.final_ln_w, self.final_ln_b, a.layer_norm_eps)
        return ops.linear(pooled, self.proj_w)

    @torch.no_grad()
    def encode(self, input_ids, attention_mask=None) -> torch.Tensor:
        """input_ids, attention_mask (n, S) -> (n, projection_dim) fp32 unit rows on the device."""
        return ops.l2_normalize_rows(self.text_embeds(input_ids, attention_mask).contiguous())
