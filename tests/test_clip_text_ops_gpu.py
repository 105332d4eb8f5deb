"""The three kernels of the packed CLIP text tower against torch: causal attention over a ragged batch (licv_attn_varlen_causal), the
token + position embedding on packed ids (licv_clip_text_embed) and the LayerNorm over selected rows (licv_layernorm_rows_fwd)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_clip_engine_gpu import close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 64
GUARD, SENTINEL = 8, -7.0


def ops():
    from licv import ops as o
    return o


def _lengths(batch):
    if batch == "edges":             # every tile boundary of the kernel (16-query sub-tiles, 32-key PV steps, the 128 limit), shuffled
        lens = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77, 127, 128]
        return [lens[i] for i in np.random.default_rng(5).permutation(len(lens))]
    return np.random.default_rng(6).integers(1, 78, 300).tolist()      # more (sequence, head) items than the GPU has compute units


@functools.lru_cache(maxsize=None)
def _case(batch, nh):
    """(qkv bf16 (total + GUARD, 3E) on the host, cu_seqlens int32, the fp32 reference (total, E)), computed once per case."""
    lens = _lengths(batch)
    cu = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    total, E = int(cu[-1]), nh * HD
    qkv = torch.randn(total + GUARD, 3 * E, generator=torch.Generator().manual_seed(100 + nh)).to(torch.bfloat16)
    ref = torch.empty(total, E)
    for s, L in zip(cu[:-1].tolist(), lens):
        q, k, v = (qkv[s:s + L, i * E:(i + 1) * E].float().view(L, nh, HD).transpose(0, 1) for i in range(3))
        sc = (q @ k.transpose(-1, -2)) * HD ** -0.5
        sc = sc.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
        ref[s:s + L] = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(L, E)
    return qkv, cu, ref


def _attn_close(out, ref):
    """The bars of tests/test_ops_gpu.py::_attn_close, restated (bf16 output, bf16 probabilities into the PV MFMA, fp32 accumulators;
    measured for that arithmetic at 2x margin)."""
    out, ref = out.float().cpu(), ref.float()
    e = (out - ref).abs()
    top = ref.abs().max()
    unit = ref.abs() * 2.0 ** -8 + top * 2.0 ** -10
    print(f"max error {float(e.max() / top):.3e} of max|ref|, {float((e / unit).max()):.3f} units")
    assert float(e.max()) <= 6e-3 * float(top), float(e.max() / top)
    assert float((e / unit).max()) <= 2.5, float((e / unit).max())


@pytest.mark.parametrize("nh", [2, 8])
@pytest.mark.parametrize("batch", ["edges", "many"])
def test_attn_varlen_causal(batch, nh):
    qkv, cu, ref = _case(batch, nh)
    total, E = ref.shape
    d_qkv, d_cu = qkv.to(DEV), cu.to(DEV)
    out = torch.full((total + GUARD, E), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops().attn_varlen_causal(d_qkv, cu, d_cu, nh, HD, HD ** -0.5, out=out)
    got = out.cpu()
    assert torch.isfinite(got.float()).all()
    assert (got[total:] == SENTINEL).all(), "rows past the last sequence were written"
    _attn_close(got[:total], ref)
    # every sequence alone: the same bits (nothing leaks across sequences, nothing depends on the batch's longest sequence)
    alone = torch.empty_like(out[:total])
    for s, e in zip(cu[:-1].tolist(), cu[1:].tolist()):
        one = torch.tensor([0, e - s], dtype=torch.int32)
        ops().attn_varlen_causal(d_qkv[s:], one, one.to(DEV), nh, HD, HD ** -0.5, out=alone[s:e])
    assert torch.equal(alone.cpu(), got[:total])


def test_attn_varlen_causal_refuses_what_it_cannot_serve():
    from licv._lib import LicvError
    call = lambda qkv, cu, nh, hd: ops().attn_varlen_causal(qkv, torch.tensor(cu, dtype=torch.int32), torch.tensor(cu, dtype=torch.int32, device=DEV),
                                                            nh, hd, hd ** -0.5)
    qkv = torch.zeros(160, 3 * 2 * HD, dtype=torch.bfloat16, device=DEV)
    call(qkv, [0, 5, 133], 2, HD)                                         # 5 and 128 tokens: served
    for cu, nh, hd, why in (([0, 5, 10], 4, 32, "head_dim 32"), ([0, 0, 5], 2, HD, "an empty sequence"), ([0, 129], 2, HD, "129 tokens"),
                            ([0, 5, 3], 2, HD, "cu_seqlens descending"), ([1, 5], 2, HD, "cu_seqlens not from 0"),
                            ([0, 100, 200], 2, HD, "more tokens than rows")):
        with pytest.raises(LicvError):
            call(qkv, cu, nh, hd)
            pytest.fail(f"accepted {why}")


@pytest.mark.parametrize("dim", [128, 512])
def test_clip_text_embed_is_the_bf16_sum_of_the_two_rows(dim):
    g = torch.Generator().manual_seed(dim)
    vocab, n_pos, total = 1000, 77, 333
    tok = torch.randn(vocab, dim, generator=g).to(torch.bfloat16)
    pos = torch.randn(n_pos, dim, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, vocab, (total,), generator=g)
    p = torch.randint(0, n_pos, (total,), generator=g).to(torch.int32)
    ids[:2], p[:2] = torch.tensor([0, vocab - 1]), torch.tensor([n_pos - 1, 0], dtype=torch.int32)
    ref = tok[ids] + pos[p.long()]
    assert ref.dtype == torch.bfloat16
    got = ops().clip_text_embed(ids.to(DEV), p.to(DEV), tok.to(DEV), pos.to(DEV))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dim", [128, 512, 100])
def test_layernorm_rows(dim):
    g = torch.Generator().manual_seed(dim)
    x = (torch.randn(200, dim, generator=g) * 2 + 0.5).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(dim, generator=g)).to(torch.bfloat16)
    b = (0.1 * torch.randn(dim, generator=g)).to(torch.bfloat16)
    rows = torch.randint(0, 200, (53,), generator=g).to(torch.int32)
    rows[:3] = torch.tensor([0, 199, 199], dtype=torch.int32)
    ref = F.layer_norm(x[rows.long()], (dim,), w, b, 1e-5)
    got = ops().layernorm_rows(x.to(DEV), rows.to(DEV), w.to(DEV), b.to(DEV), 1e-5)
    close_bf16(got, ref, exact_frac=0.98)
