"""licv_attn_fwd_ragged (csrc/attention.hip): the tiled attention on PACKED rows of a right-padded batch against licv_attn_fwd on the
padded batch itself.  Key tiles (64) and query blocks (64 per workgroup, 128 = two of them) keep their boundaries relative to the
sequence start, so every real row must come out with the SAME BITS; rows of the output buffer past `total` must not be written.
Lengths sit on each side of the 64-key tile edge and of the 128-query edge."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0
NH = 2


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    host = torch.tensor(cu, dtype=torch.int32)
    return host, host.to(DEV)


def _real_rows(lens, S):
    return torch.cat([torch.arange(n) + b * S for b, n in enumerate(lens)]).to(DEV)


@pytest.mark.parametrize("hd", [16, 32, 64, 80, 96, 128])
def test_causal_packed_rows_have_the_bits_of_the_padded_batch(hd):
    from licv import ops
    lens = [1, 63, 64, 65, 127, 128, 129, 200]
    B, S, E = len(lens), max(lens), NH * hd
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(B, S, 3 * E, generator=g).to(torch.bfloat16).to(DEV)
    key_valid = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).to(torch.int32).to(DEV).contiguous()
    flat = qkv.view(-1)
    want = ops.attention(flat, flat[E:], flat[2 * E:], B, S, S, NH, NH, hd, S * 3 * E, 3 * E, S * 3 * E, 3 * E, hd ** -0.5, 1, key_valid=key_valid)
    rows = _real_rows(lens, S)
    total = int(rows.numel())
    packed = qkv.view(B * S, 3 * E)[rows].contiguous().view(-1)
    cu_host, cu_dev = _cu(lens)
    out = torch.full((total + 7, E), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.attention_ragged(packed, packed[E:], packed[2 * E:], cu_host, cu_dev, 0, NH, NH, hd, 3 * E, 0, 3 * E, hd ** -0.5, 1, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[:total], want.view(B * S, E)[rows])
    assert bool((out[total:] == SENTINEL).all()), "rows past total were written"


@pytest.mark.parametrize("hd", [64, 128])
def test_image_mask_packed_rows_have_the_bits_of_the_padded_batch(hd):
    from licv import ops
    lens, img_len, n_img = [5, 128, 129, 190], 64, 3
    B, S, E, Nk = len(lens), max(lens), NH * hd, img_len * n_img
    g = torch.Generator().manual_seed(100 + hd)
    q = torch.randn(B, S, E, generator=g).to(torch.bfloat16).to(DEV)
    kv = torch.randn(B, Nk, 2 * E, generator=g).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, n_img + 1, (B, S), generator=g)                    # n_img = the token attends no image (a row of zeros)
    img_mask = (which[..., None] == torch.arange(n_img)).to(torch.int32).to(DEV).contiguous()
    kvf = kv.view(-1)
    want = ops.attention(q.view(-1), kvf, kvf[E:], B, S, Nk, NH, NH, hd, S * E, E, Nk * 2 * E, 2 * E, hd ** -0.5, 3, img_mask=img_mask, img_len=img_len)
    rows = _real_rows(lens, S)
    total = int(rows.numel())
    cu_host, cu_dev = _cu(lens)
    out = torch.full((total + 7, E), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.attention_ragged(q.view(B * S, E)[rows].contiguous().view(-1), kvf, kvf[E:], cu_host, cu_dev, Nk, NH, NH, hd, E, Nk * 2 * E, 2 * E,
                         hd ** -0.5, 3, img_mask=img_mask.view(B * S, n_img)[rows].contiguous(), img_len=img_len, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[:total], want.view(B * S, E)[rows])
    assert bool((out[total:] == SENTINEL).all()), "rows past total were written"


def test_bad_cu_seqlens_are_refused_before_any_launch():
    from licv import _lib
    from licv._lib import AttnArgs
    hd, E = 64, NH * 64
    qkv = torch.zeros(16, 3 * E, dtype=torch.bfloat16, device=DEV)
    out = torch.full((16, E), SENTINEL, dtype=torch.bfloat16, device=DEV)
    a = AttnArgs()
    a.q, a.q_bs, a.q_rs = qkv.data_ptr(), 0, 3 * E
    a.k, a.v, a.kv_bs, a.kv_rs = qkv.data_ptr() + 2 * E, qkv.data_ptr() + 4 * E, 0, 3 * E
    a.o = out.data_ptr()
    a.B, a.Sq, a.Sk, a.n_heads, a.n_kv_heads, a.head_dim = 2, 0, 0, NH, NH, hd
    a.scale, a.mask_mode, a.key_valid, a.img_mask, a.n_img, a.img_len = hd ** -0.5, 1, None, None, 0, 0
    fn = _lib.lib().licv_attn_fwd_ragged
    good_host, good_dev = _cu([8, 8])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for name, cu in (("not ascending", [0, 9, 4]), ("a zero length", [0, 8, 8]), ("not from 0", [1, 8, 16])):
        host = torch.tensor(cu, dtype=torch.int32)
        assert fn(C.byref(a), ptr(host), ptr(host.to(DEV)), None) == _lib_badarg(), name
    assert fn(C.byref(a), ptr(good_host), None, None) == _lib_badarg(), "device copy missing"
    assert fn(C.byref(a), None, ptr(good_dev), None) == _lib_badarg(), "host copy missing"
    a.mask_mode = 0
    assert fn(C.byref(a), ptr(good_host), ptr(good_dev), None) == _lib_badarg(), "mask mode 0"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call launched something"


def _lib_badarg() -> int:
    return -1            # LICV_E_BADARG (include/licv_hip.h)
