"""The model pieces the engines share, each written once: the pre-LN encoder layer of the four towers (ViT-H, SigLIP, CLIP image and
text) and its weight loader, causal self-attention with its KV-cache cases, the batch-slice fan-out over HIP streams, and the small
tails (rotary tables, the logits view, the hook arguments).  Plain functions over ``licv.ops``: every engine keeps its own layer loop."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from . import ops

# From this many rows on the text stacks fold the residual adds into the norm that follows and take fp8 operands (where the weights
# carry them), and the SigLIP tower takes fp8 operands.  csrc/runner.hip holds the same number for the native layer runner.
FOLD_MIN_ROWS = 512


def bf16_on(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.bfloat16).contiguous()


def pad_cols(w: torch.Tensor, to: int) -> torch.Tensor:
    if w.shape[1] == to:
        return w.contiguous()
    out = torch.zeros((w.shape[0], to), dtype=w.dtype, device=w.device)
    out[:, : w.shape[1]] = w
    return out


def rotary_tables(head_dim: int, base: float, n_positions: int, dev):
    """(cos, sin) bf16 (n_positions, head_dim): fp32 inv_freq and angles, cast to the model dtype (hf:idefics/modeling_idefics.py:357-379,
    hf:mistral/modeling_mistral.py MistralRotaryEmbedding)."""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    emb = torch.cat((torch.outer(torch.arange(n_positions, dtype=torch.float), inv),) * 2, dim=-1)
    return bf16_on(emb.cos(), dev), bf16_on(emb.sin(), dev)


# ------------------------------------------------------------------------------------------------ pre-LN encoder layer
@dataclass
class EncoderLayer:
    ln1_w: torch.Tensor; ln1_b: torch.Tensor; qkv_w: torch.Tensor; qkv_b: torch.Tensor
    out_w: torch.Tensor; out_b: torch.Tensor; ln2_w: torch.Tensor; ln2_b: torch.Tensor
    fc1_w: torch.Tensor; fc1_b: torch.Tensor; fc2_w: torch.Tensor; fc2_b: torch.Tensor
    q8: Optional[dict] = None           # fp8 copies of the four projection weights (Idefics2Weights, fp8_vision)


def load_encoder_layers(g: Callable[[str], torch.Tensor], prefix: str, n_layers: int, pad_inter: Optional[int] = None) -> List[EncoderLayer]:
    """Layers `prefix`0. .. `prefix`{n_layers-1}. of an HF CLIP / SigLIP encoder through `g` (key -> device tensor), Q | K | V fused.
    pad_inter: the MLP width padded to it with zero fc1 rows / bias and zero fc2 columns (act(0) = 0: the result is unchanged)."""
    def pad_rows(t):
        out = torch.zeros((pad_inter, *t.shape[1:]), dtype=t.dtype, device=t.device)
        out[: t.shape[0]] = t
        return out
    layers = []
    for i in range(n_layers):
        p = f"{prefix}{i}."
        cat = lambda suf: torch.cat([g(p + f"self_attn.{n}_proj.{suf}") for n in ("q", "k", "v")]).contiguous()
        fc1_w, fc1_b, fc2_w = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias"), g(p + "mlp.fc2.weight")
        if pad_inter is not None:
            fc1_w, fc1_b, fc2_w = pad_rows(fc1_w), pad_rows(fc1_b), pad_cols(fc2_w, pad_inter)
        layers.append(EncoderLayer(g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), cat("weight"), cat("bias"),
                                   g(p + "self_attn.out_proj.weight"), g(p + "self_attn.out_proj.bias"),
                                   g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), fc1_w, fc1_b, fc2_w, g(p + "mlp.fc2.bias")))
    return layers


def dense_attend(n: int, T: int, n_heads: int, head_dim: int, mode: int = 0, key_valid: Optional[torch.Tensor] = None):
    """The `attend` of a tower whose n images hold T tokens each: unmasked (mode 0) or under a per-image key-valid mask (mode 2)."""
    E = n_heads * head_dim
    return lambda qkv: ops.attention(qkv, qkv.view(-1)[E:], qkv.view(-1)[2 * E:], n, T, T, n_heads, n_heads, head_dim,
                                     T * 3 * E, 3 * E, T * 3 * E, 3 * E, head_dim ** -0.5, mode, key_valid=key_valid)


def encoder_layer_(x: torch.Tensor, L: EncoderLayer, eps: float, act: str, attend, fp8: bool = False) -> None:
    """x (rows, E) bf16 <- one pre-LN layer, in place: LayerNorm, fused QKV GEMM with bias, attend(qkv) -> o, out-projection with
    residual, LayerNorm, fc1 with `act`, fc2 with residual.  act: an epilogue activation of ops.linear, or "quick_gelu" (CLIP: its own
    kernel after fc1).  fp8: e4m3 operands for the four projections; the LayerNorms write the fp8 rows themselves, no bf16 copy."""
    if fp8:
        qkv = ops.linear_fp8(*ops.layernorm_q8(x, L.ln1_w, L.ln1_b, eps), *L.q8["qkv_w"], bias=L.qkv_b)
    else:
        qkv = ops.linear(ops.layernorm(x, L.ln1_w, L.ln1_b, eps), L.qkv_w, bias=L.qkv_b)
    o = attend(qkv)
    del qkv                                                                # freed before the MLP's buffers are taken
    if fp8:
        ops.linear_fp8(*ops.quantize_fp8(o.view(x.shape)), *L.q8["out_w"], bias=L.out_b, residual=x, out=x)
        y = ops.linear_fp8(*ops.layernorm_q8(x, L.ln2_w, L.ln2_b, eps), *L.q8["fc1_w"], bias=L.fc1_b, act=act)
        ops.linear_fp8(*ops.quantize_fp8(y), *L.q8["fc2_w"], bias=L.fc2_b, residual=x, out=x)
        return
    ops.linear(o.view(x.shape), L.out_w, bias=L.out_b, residual=x, out=x)
    y = ops.layernorm(x, L.ln2_w, L.ln2_b, eps)
    if act == "quick_gelu":
        y = ops.quick_gelu_(ops.linear(y, L.fc1_w, bias=L.fc1_b))
    else:
        y = ops.linear(y, L.fc1_w, bias=L.fc1_b, act=act)
    ops.linear(y, L.fc2_w, bias=L.fc2_b, residual=x, out=x)


# ------------------------------------------------------------------------------------------------ text stacks
def causal_self_attention(project, x, qkv_w: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                          key_valid: torch.Tensor, B: int, S: int, n_heads: int, n_kv_heads: int, head_dim: int, rotary,
                          cache: Optional[torch.Tensor] = None, kv_rows: Optional[torch.Tensor] = None, past: int = 0,
                          append: bool = True):
    """Rotary + causal attention of one decoder layer on the fused projection [Q | K | V] of the normed rows x: (o, rotated qkv).
    project() -> the (B * S, (n_heads + 2 n_kv_heads) * head_dim) bf16 rows x @ qkv_w.T, by whichever GEMM the caller routes it to.
    rotary = (n_heads, tensor_stride, n_tensors) of the ops.rotary_ launch over Q and K.  cache: this layer's (rows, max_len, [K | V])
    tensor or None.  No cache: attention among the S new tokens.  Cache and S > 1 (prefill): K | V appended at `past`, attention over
    the cache.  Cache and S == 1 (a decode step): rotary + append + attention in one launch, fed by the split-K slices of the
    projection where the plan splits it; no qkv tensor exists then (None).  Cache, a row table and S > 1 (a continuation step of S
    tokens per row behind shared history): rotary + attention through the table in one launch (ops.append_attn); `append` says whether
    the S tokens' K | V go into the row's own cache row - a scoring pass leaves the cache as it found it, also when S == 1 (the decode
    launch always appends, and the rows of a scoring pass have no cache row of their own).  No rotated qkv exists (None)."""
    nh, nkv, hd = n_heads, n_kv_heads, head_dim
    qd, kd = nh * hd, nkv * hd
    ldq = qd + 2 * kd
    if cache is not None and kv_rows is not None and (S > 1 or not append):
        return ops.append_attn(project(), cos, sin, pos, cache, past, S, nh, nkv, hd, hd ** -0.5, key_valid=key_valid, kv_rows=kv_rows,
                               append=append), None
    if cache is not None and S == 1:
        qs = ops.linear_produce(x, qkv_w) if not isinstance(x, tuple) else None
        min_keys, n_splits = ops.decode_split_settings()
        if past + 1 >= min_keys:                          # a long history (by default: one decode_attn refuses): split keys + merge
            return ops.decode_attn_split(qs if qs is not None else project(), cos, sin, pos, cache, past, nh, nkv, hd, hd ** -0.5,
                                         key_valid=key_valid, kv_rows=kv_rows, n_splits=n_splits), None
        return ops.decode_attn(qs if qs is not None else project(), cos, sin, pos, cache, past, nh, nkv, hd, hd ** -0.5,
                               key_valid=key_valid, kv_rows=kv_rows), None
    qkv = project()
    ops.rotary_(qkv, cos, sin, pos, B * S, rotary[0], hd, ldq, rotary[1], rotary[2])
    if cache is None:
        o = ops.attention(qkv, qkv.view(-1)[qd:], qkv.view(-1)[qd + kd:], B, S, S, nh, nkv, hd, S * ldq, ldq, S * ldq, ldq,
                          hd ** -0.5, 1, key_valid=key_valid)
    else:
        cache[:, past:past + S] = qkv.view(B, S, ldq)[:, :, qd:]                    # append K|V (device copy)
        o = ops.attention(qkv, cache, cache.view(-1)[kd:], B, S, past + S, nh, nkv, hd, S * ldq, ldq, cache.shape[1] * 2 * kd, 2 * kd,
                          hd ** -0.5, 1, key_valid=key_valid)
    return o, qkv


def hook_args(icv: Optional[torch.Tensor], alpha: Optional[torch.Tensor], hook_layers: Optional[Sequence[int]], dev):
    """(hook slot of every hooked layer id, icv, alpha), the two tensors as the hook kernels take them: fp32, contiguous, on `dev`."""
    idx_of = {int(l): i for i, l in enumerate(hook_layers)} if (icv is not None and hook_layers is not None) else {}
    if icv is not None:
        icv = icv.detach().to(device=dev, dtype=torch.float32).contiguous()
        if alpha is not None:
            alpha = alpha.detach().to(device=dev, dtype=torch.float32).contiguous()
    return idx_of, icv, alpha


def logits_view(logits: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """(B * S, V) rows with a (possibly padded) row stride -> the (B, S, V) view over them."""
    V = logits.shape[-1]
    return logits.view(B, S, V) if logits.is_contiguous() else logits.as_strided((B, S, V), (S * logits.stride(0), logits.stride(0), 1))


def lm_logits(x: torch.Tensor, head: torch.Tensor, B: int, S: int, logits_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The LM head on the final-normed rows: (B, S, V), or (n_rows, V) for the flat rows b * S + s in `logits_rows` only."""
    if logits_rows is not None:
        return ops.linear(x.index_select(0, logits_rows), head)
    return logits_view(ops.linear(x, head), B, S)


# ------------------------------------------------------------------------------------------------ batch slices
def run_slices(streams: list, dev, n_slices: int, run_slice, skip=()) -> list:
    """run_slice(i) for every slice i not in `skip`, each on a HIP stream of its own (`streams`, grown as needed and kept by the
    caller), joined on the caller's stream: the outputs in slice order, for the caller to concatenate."""
    cur = torch.cuda.current_stream(dev)
    while len(streams) < n_slices:
        streams.append(torch.cuda.Stream(device=dev))
    outs = []
    for i in range(n_slices):
        if i in skip:
            continue
        streams[i].wait_stream(cur)                                        # the inputs were produced on the caller's stream
        with torch.cuda.stream(streams[i]):
            outs.append(run_slice(i))
    for i in range(n_slices):
        cur.wait_stream(streams[i])
    for o in outs:
        o.record_stream(cur)                                               # allocated on a side stream, read on the caller's from here on
    return outs
