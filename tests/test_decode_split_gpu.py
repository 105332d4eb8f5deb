"""licv_decode_attn_split (csrc/decode_split.hip): a decode step's rotary + KV append + attention with the key range of every
(row, kv head) cut into splits and a merge launch behind it, against (a) licv_decode_attn on the same inputs — the cache bit for bit
for every split count, the output bit for bit for one split — and (b) the oracle's arithmetic as tests/test_decode_attn_gpu.py
states it: rotary with every bf16 op rounded, attention in fp64 on the rounded operands, bar 2 bf16 ulp of the output scale
(2 * 2^-8 * max|ref|, the bar licv_decode_attn is held to).  With more than one split the output may differ from licv_decode_attn's
in the last place (the merge rescales every partial by exp2(m_s - max m) where the single launch rescales sweep by sweep), so both
are held to the same bar of the reference and to the same bar of each other.  Beyond 10 240 keys only (b) exists: the single launch
refuses such a history."""
import functools

import pytest
import torch

from oracle import idefics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2 * 2.0 ** -8


def _inputs(M, nh, nkv, hd, past, from_slices, R_rows, seed):
    """Random inputs of one decode step (CPU tensors): the fused QKV rows as bf16 and, when asked, as three fp32 slices whose sum in
    slice order rounds to them; tables; a cache; a random row table whose entry at `past` is the row's own cache row; a random mask."""
    g = torch.Generator().manual_seed(seed)
    qd, kd = nh * hd, nkv * hd
    ldq = qd + 2 * kd
    if from_slices:
        sl = torch.randn(3, M, ldq, generator=g) * 3 ** -0.5
        qkv = ((sl[0] + sl[1]) + sl[2]).to(torch.bfloat16)              # fp32 adds in slice order from 0.f, then one rounding
    else:
        sl = None
        qkv = torch.randn(M, ldq, generator=g).to(torch.bfloat16)
    n_pos, max_len = 256, past + 4
    cos, sin = R.rotary_tables(hd, n_pos, 10000.0, torch.bfloat16)
    pos = torch.randint(0, n_pos, (M,), generator=g)
    cache0 = torch.randn(R_rows, max_len, 2 * kd, generator=g).to(torch.bfloat16)
    rows = torch.randint(0, R_rows, (M, max_len), generator=g).to(torch.int32)
    rows[:, past] = torch.arange(M, dtype=torch.int32)                  # a row's own new token lives in its own cache row
    valid = (torch.rand(M, past + 1, generator=g) > 0.2).to(torch.int32)
    valid[:, past] = 1
    return dict(qkv=qkv, slices=sl, cos=cos, sin=sin, pos=pos, cache0=cache0, rows=rows, valid=valid)


def _src(z):
    from licv import ops
    if z["slices"] is None:
        return z["qkv"].to(DEV)
    sl = z["slices"].to(DEV).contiguous()
    _, M, ldq = sl.shape
    return ops.Slices(sl, 3, M * ldq, ldq, M, ldq)


def _oracle(z, M, nh, nkv, hd, past):
    """(K | V of the new token as the oracle's rotary gives it, fp64 attention output) - computed once per case."""
    qd, kd, rep = nh * hd, nkv * hd, nh // nkv
    x, pos, rows, valid = z["qkv"], z["pos"], z["rows"], z["valid"]
    q = x[:, :qd].view(M, 1, nh, hd).transpose(1, 2)
    k = x[:, qd:qd + kd].view(M, 1, nkv, hd).transpose(1, 2)
    v = x[:, qd + kd:].view(M, nkv, hd)
    cs, sn = z["cos"][pos].view(M, 1, 1, hd), z["sin"][pos].view(M, 1, 1, hd)
    qr = (q * cs) + (R.rotate_half(q) * sn)
    kr = (k * cs) + (R.rotate_half(k) * sn)
    new_kv = torch.cat([kr.reshape(M, kd), v.reshape(M, kd)], 1)
    hist = z["cache0"].clone()
    hist[:M, past] = new_kv
    jj = torch.arange(past + 1)
    G = hist[rows[:, : past + 1].long(), jj[None, :]]                                     # (M, Sk, 2kd) through the row table
    Kh, Vh = G[..., :kd].reshape(M, past + 1, nkv, hd).double(), G[..., kd:].reshape(M, past + 1, nkv, hd).double()
    s = torch.einsum("mgrd,mjgd->mgrj", qr.reshape(M, nkv, rep, hd).double(), Kh) * hd ** -0.5
    s = s.masked_fill(valid[:, None, None, :] == 0, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)                              # a row with no visible key: 0, as the kernel
    ref = torch.einsum("mgrj,mjgd->mgrd", p, Vh).reshape(M, qd)
    return new_kv, ref


def _call(z, M, nh, nkv, hd, past, n_splits, fn=None):
    from licv import ops
    cache = z["cache0"].clone().to(DEV)
    kw = dict(key_valid=z["valid"].to(DEV), kv_rows=z["rows"].to(DEV))
    args = (_src(z), z["cos"].to(DEV), z["sin"].to(DEV), z["pos"].to(DEV), cache, past, nh, nkv, hd, hd ** -0.5)
    out = ops.decode_attn(*args, **kw) if n_splits == "single" else ops.decode_attn_split(*args, **kw, n_splits=n_splits)
    return out.cpu(), cache.cpu()


SHORT = [(6, 4, 2, 64, 0), (5, 4, 4, 96, 63), (9, 8, 8, 128, 64), (24, 32, 8, 128, 130), (9, 8, 8, 128, 200)]


@functools.lru_cache(maxsize=None)
def _short_case(M, nh, nkv, hd, past, from_slices):
    z = _inputs(M, nh, nkv, hd, past, from_slices, M + 3, M * 1000 + past)
    if M > 2:
        z["valid"][2, : max(past - 1, 0)] = 0                           # a row that sees (almost) only its own token
    new_kv, ref = _oracle(z, M, nh, nkv, hd, past)
    out1, cache1 = _call(z, M, nh, nkv, hd, past, "single")
    return z, new_kv, ref, out1, cache1


@pytest.mark.parametrize("n_splits", [1, 2, 3, 7])
@pytest.mark.parametrize("from_slices", [False, True], ids=["bf16_rows", "split_k_slices"])
@pytest.mark.parametrize("M,nh,nkv,hd,past", SHORT)
def test_forced_splits_on_short_histories(M, nh, nkv, hd, past, from_slices, n_splits):
    z, new_kv, ref, out1, cache1 = _short_case(M, nh, nkv, hd, past, from_slices)
    out, cache = _call(z, M, nh, nkv, hd, past, n_splits)              # 7 exceeds the sweep count of every shape here: clamped
    scale = float(ref.abs().max())
    assert torch.equal(cache1[:M, past], new_kv), "licv_decode_attn's appended K | V (the yardstick of this test)"
    assert torch.equal(cache, cache1), "the cache after the split form, bit for bit the single launch's"
    d = (out.double() - out1.double()).abs()
    print(f"\n  n_splits={n_splits}: {float((d == 0).double().mean()):.4f} of the output elements bit-equal to licv_decode_attn")
    if n_splits == 1 or past < 64:                                      # one split (asked for, or clamped to the one sweep): the same bits
        assert torch.equal(out, out1)
    err = float((out.double() - ref).abs().max())
    assert err <= BAR * scale, f"split decode attention vs fp64: {err:.3e} at scale {scale:.3e}"
    assert float(d.max()) <= BAR * scale, f"split form vs single launch: {float(d.max()):.3e} at scale {scale:.3e}"


LONG = (3, 4, 2, 128, 10300)


@functools.lru_cache(maxsize=None)
def _long_case():
    M, nh, nkv, hd, past = LONG
    z = _inputs(M, nh, nkv, hd, past, False, 5, 4242)
    z["valid"][0, :9000] = 0                                            # several splits of row 0 are wholly masked
    z["valid"][2, :past] = 0                                            # row 2 sees only its own key
    new_kv, ref = _oracle(z, M, nh, nkv, hd, past)
    return z, new_kv, ref


@pytest.mark.parametrize("n_splits", [None, 32], ids=["plan", "32"])
def test_beyond_the_single_launch_limit(n_splits):
    from licv import _lib, ops
    M, nh, nkv, hd, past = LONG
    z, new_kv, ref = _long_case()
    with pytest.raises(_lib.LicvError, match="LDS budget"):             # the single launch refuses this history
        _call(z, M, nh, nkv, hd, past, "single")
    if n_splits is None:
        assert ops.decode_attn_split_plan(M, nh, nkv, hd, past + 1)[0] > 1
    out, cache = _call(z, M, nh, nkv, hd, past, n_splits)
    scale = float(ref.abs().max())
    err = float((out.double() - ref).abs().max())
    print(f"\n  {past + 1} keys, n_splits={n_splits}: max|out - fp64| = {err:.3e}, bar {BAR * scale:.3e}")
    assert err <= BAR * scale, f"split decode attention vs fp64: {err:.3e} at scale {scale:.3e}"
    assert torch.equal(cache[:M, past], new_kv), "K (rotated) | V of the new token as appended to the cache"
    keep = torch.ones(cache.shape[:2], dtype=torch.bool)
    keep[:M, past] = False
    assert torch.equal(cache[keep], z["cache0"][keep]), "nothing else in the cache may change"
    out2, cache2 = _call(z, M, nh, nkv, hd, past, n_splits)             # a fresh copy of cache0: the appended key comes from registers again
    assert torch.equal(out2, out) and torch.equal(cache2, cache)


@pytest.mark.parametrize("n_splits", [1, 3])
def test_rows_without_visible_history_and_without_any_visible_key(n_splits):
    M, nh, nkv, hd, past = 4, 4, 2, 128, 150
    z = _inputs(M, nh, nkv, hd, past, False, M + 2, 99)
    z["cache0"][M + 1] = float("nan")                                   # a cache row that no visible key selects ...
    z["rows"][z["rows"] == M + 1] = 0
    z["valid"][0, :past] = 0                                            # row 0: every key masked but its own
    z["valid"][1, :] = 0                                                # row 1: every key masked, its own included
    z["rows"][:2, :past] = M + 1                                        # ... and their masked keys point at it
    out, cache = _call(z, M, nh, nkv, hd, past, n_splits)
    assert torch.isfinite(out.float()).all()
    assert bool((out[1] == 0).all()), "no visible key: L = 0, the output row is 0"
    kd, rep = nkv * hd, nh // nkv
    v_new = z["qkv"][0, nh * hd + kd:].view(nkv, 1, hd).expand(nkv, rep, hd).reshape(nh * hd)
    assert torch.equal(out[0], v_new), "only its own key: P = 1, the output is the new token's V"
    new_kv, ref = _oracle(z, M, nh, nkv, hd, past)
    assert float((out[2:].double() - ref[2:]).abs().max()) <= BAR * float(ref[2:].abs().max())
