"""licv_append_attn (csrc/append_attn.hip): a continuation step of T new tokens per row through the cache-row table in one launch,
against (a) the oracle's arithmetic as tests/test_decode_attn_gpu.py builds it - rotary with every bf16 op rounded
(oracle/idefics_ref, bit for bit into the cache), attention in fp64 on the rounded operands, bar 2 bf16 ulp of the output scale - and
(b) the chain of T licv_decode_attn steps it replaces.  Random row table and key mask, with one row that sees almost nothing but its
own tokens.  Also: the cache with and without append, T = 1 against the decode kernel bit for bit, padded tails, causality, and the
identity row table."""
import functools

import pytest
import torch

from oracle import idefics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(6, 4, 2, 64, 5, 5), (5, 4, 4, 96, 0, 3), (7, 4, 4, 16, 9, 4), (9, 8, 8, 128, 62, 5),      # 62 + 5: the new tokens straddle a sweep
          (24, 32, 8, 128, 101, 16), (12, 32, 32, 128, 200, 32)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(M, nh, nkv, hd, past, T):
    """Inputs (CPU) and the two references, computed once per shape and never modified."""
    g = torch.Generator().manual_seed(M * 1000 + past * 7 + T)
    qd, kd = nh * hd, nkv * hd
    ldq = qd + 2 * kd
    qkv = torch.randn(M * T, ldq, generator=g).to(torch.bfloat16)
    n_pos, max_len, R_rows = 320, past + T + 3, M + 3
    cos, sin = R.rotary_tables(hd, n_pos, 10000.0, torch.bfloat16)
    pos = torch.randint(0, n_pos, (M * T,), generator=g)
    cache0 = torch.randn(R_rows, max_len, 2 * kd, generator=g).to(torch.bfloat16)
    rows = torch.randint(0, R_rows, (M, max_len), generator=g).to(torch.int32)
    rows[:, past:] = torch.arange(M, dtype=torch.int32)[:, None]          # (the chain of decode steps appends into the row's own cache row)
    valid = (torch.rand(M, past + T, generator=g) > 0.2).to(torch.int32)
    valid[:, past:] = 1
    if M > 2:
        valid[2, : max(past - 1, 0)] = 0                                   # a row that sees (almost) only its own tokens
    # ---- the oracle's arithmetic
    q = qkv[:, :qd].view(M * T, 1, nh, hd).transpose(1, 2)
    k = qkv[:, qd:qd + kd].view(M * T, 1, nkv, hd).transpose(1, 2)
    v = qkv[:, qd + kd:].view(M * T, nkv, hd)
    cs, sn = cos[pos].view(M * T, 1, 1, hd), sin[pos].view(M * T, 1, 1, hd)
    qr = (q * cs) + (R.rotate_half(q) * sn)
    kr = (k * cs) + (R.rotate_half(k) * sn)
    new_kv = torch.cat([kr.reshape(M * T, kd), v.reshape(M * T, kd)], 1).view(M, T, 2 * kd)
    Sk = past + T
    jj = torch.arange(past)
    hist = cache0[rows[:, :past].long(), jj[None, :]]                     # (M, past, 2kd) through the row table
    keys = torch.cat([hist, new_kv], 1)                                    # (M, Sk, 2kd)
    rep = nh // nkv
    Kh = keys[..., :kd].reshape(M, Sk, nkv, hd).repeat_interleave(rep, 2).double()
    Vh = keys[..., kd:].reshape(M, Sk, nkv, hd).repeat_interleave(rep, 2).double()
    s = torch.einsum("mthd,mjhd->mhtj", qr.reshape(M, T, nh, hd).double(), Kh) * hd ** -0.5
    vis = (torch.arange(Sk)[None, :] <= past + torch.arange(T)[:, None])   # (T, Sk)
    s = s.masked_fill(~(vis[None, None] & (valid[:, None, None, :] != 0)), float("-inf"))
    ref = torch.einsum("mhtj,mjhd->mthd", torch.softmax(s, -1), Vh).reshape(M * T, qd)
    return dict(qkv=qkv, cos=cos, sin=sin, pos=pos, cache0=cache0, rows=rows, valid=valid, new_kv=new_kv, ref=ref,
                dims=(M, nh, nkv, hd, past, T))


def _run(c, append=True, T=None, qkv=None, valid="case", rows="case", pos=None, cache=None):
    from licv import ops
    M, nh, nkv, hd, past, T0 = c["dims"]
    T = T0 if T is None else T
    cache = c["cache0"].clone().to(DEV) if cache is None else cache
    valid = c["valid"] if isinstance(valid, str) else valid
    rows = c["rows"] if isinstance(rows, str) else rows
    out = ops.append_attn((c["qkv"] if qkv is None else qkv).to(DEV), c["cos"].to(DEV), c["sin"].to(DEV), (c["pos"] if pos is None else pos).to(DEV),
                          cache, past, T, nh, nkv, hd, hd ** -0.5, key_valid=None if valid is None else valid.contiguous().to(DEV),
                          kv_rows=None if rows is None else rows.to(DEV), append=append)
    return out.cpu(), cache.cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_append_attn_matches_fp64_and_leaves_the_cache_as_stated(shape):
    c = _case(*shape)
    M, nh, nkv, hd, past, T = shape
    ref = c["ref"]
    bar = 2 * 2.0 ** -8 * float(ref.abs().max())
    out, got = _run(c, append=True)
    err = float((out.double() - ref).abs().max())
    print(f"append_attn vs fp64: {err:.3e} (bar {bar:.3e})")
    assert err <= bar, f"append attention vs fp64: {err:.3e} at scale {float(ref.abs().max()):.3e}"
    assert torch.equal(got[:M, past:past + T], c["new_kv"]), "K (rotated) | V of the new tokens as appended to the cache"
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[:M, past:past + T] = False
    assert torch.equal(got[keep], c["cache0"][keep]), "nothing else in the cache may change"
    out0, got0 = _run(c, append=False)
    assert torch.equal(got0, c["cache0"]), "append = 0 must not write the cache"
    assert torch.equal(out0, out), "the output does not depend on append"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_append_attn_against_the_chain_of_decode_steps(shape):
    from licv import ops
    c = _case(*shape)
    M, nh, nkv, hd, past, T = shape
    qd = nh * hd
    out, got = _run(c, append=True)
    cache = c["cache0"].clone().to(DEV)
    cos, sin, rows = c["cos"].to(DEV), c["sin"].to(DEV), c["rows"].to(DEV)
    qkv, pos = c["qkv"].view(M, T, -1), c["pos"].view(M, T)
    chain = torch.empty(M, T, qd, dtype=torch.bfloat16)
    for t in range(T):
        o = ops.decode_attn(qkv[:, t].contiguous().to(DEV), cos, sin, pos[:, t].contiguous().to(DEV), cache, past + t, nh, nkv, hd, hd ** -0.5,
                            key_valid=c["valid"][:, : past + t + 1].contiguous().to(DEV), kv_rows=rows)
        chain[:, t] = o.cpu()
    d = (out.float() - chain.view(M * T, qd).float()).abs()
    bar = 2 * 2.0 ** -8 * float(c["ref"].abs().max())
    print(f"append_attn vs decode chain: max {float(d.max()):.3e} (bar {bar:.3e}), bit-equal share {float((d == 0).float().mean()):.4f}")
    assert float(d.max()) <= bar
    assert torch.equal(cache.cpu(), got), "the chain and the single launch leave the same cache"


@pytest.mark.parametrize("M,nh,nkv,hd,past", [(24, 32, 32, 128, 36), (24, 32, 8, 128, 101), (6, 4, 2, 64, 5), (9, 8, 8, 128, 200), (5, 4, 4, 96, 0)])
def test_one_token_is_the_decode_kernel_bit_for_bit(M, nh, nkv, hd, past):
    from licv import ops
    c = _case(M, nh, nkv, hd, past, 1)
    out, got = _run(c, append=True)
    cache = c["cache0"].clone().to(DEV)
    o = ops.decode_attn(c["qkv"].to(DEV), c["cos"].to(DEV), c["sin"].to(DEV), c["pos"].to(DEV), cache, past, nh, nkv, hd, hd ** -0.5,
                        key_valid=c["valid"].to(DEV), kv_rows=c["rows"].to(DEV))
    assert torch.equal(out, o.cpu()) and torch.equal(got, cache.cpu())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_padding_does_not_leak(shape):
    c = _case(*shape)
    M, nh, nkv, hd, past, T = shape
    n = T - 2
    valid = c["valid"].clone()
    valid[:, past + n:] = 0                                                # every row's last T - n tokens are padding
    full, _ = _run(c, append=False, valid=valid)
    assert torch.isfinite(full.float()).all(), "a padded query's output is unspecified but finite"
    qkv_n = c["qkv"].view(M, T, -1)[:, :n].reshape(M * n, -1).contiguous()
    pos_n = c["pos"].view(M, T)[:, :n].reshape(-1).contiguous()
    short, _ = _run(c, append=False, T=n, qkv=qkv_n, pos=pos_n, valid=valid[:, : past + n])
    assert torch.equal(full.view(M, T, -1)[:, :n], short.view(M, n, -1))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_causality(shape):
    c = _case(*shape)
    M, nh, nkv, hd, past, T = shape
    base, _ = _run(c, append=False)
    u = T // 2
    qkv = c["qkv"].clone().view(M, T, -1)
    qkv[:, u] = torch.randn(qkv[:, u].shape, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    out, _ = _run(c, append=False, qkv=qkv.view(M * T, -1))
    a, b = base.view(M, T, -1), out.view(M, T, -1)
    assert torch.equal(a[:, :u], b[:, :u]), "token u changed an earlier token's output"
    assert not torch.equal(a[:, u:], b[:, u:])


def test_no_row_table_is_the_identity_table():
    c = _case(6, 4, 2, 64, 5, 5)
    M, past, T = 6, 5, 5
    own = torch.arange(M, dtype=torch.int32).unsqueeze(1).repeat(1, c["rows"].shape[1])
    o1, c1 = _run(c, rows=None)
    o2, c2 = _run(c, rows=own)
    assert torch.equal(o1, o2) and torch.equal(c1, c2)
