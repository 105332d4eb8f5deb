"""licv_decode_attn_split_plan / licv_decode_attn_split at the ABI: both symbols are declared and exported, the plan is a pure function
with the documented bounds and workspace size, and argument errors come back from the host before any launch (no GPU needed: every
call here must return before it reaches one)."""
import ctypes
import re

import pytest

from licv import _lib


def _plan(M, nh, nkv, hd, Sk):
    n = ctypes.c_int(-7)
    nbytes = _lib.lib().licv_decode_attn_split_plan(M, nh, nkv, hd, Sk, ctypes.byref(n))
    return n.value, nbytes


def _good(past=200):
    a = _lib.DecodeAttnArgs()
    a.qkv_bf16 = a.cos = a.sin = a.position_ids = a.cache = a.out = 4096          # never dereferenced on the host
    a.ldq, a.n_pos, a.max_len, a.past = 3 * 256, 64, past + 4, past
    a.M, a.n_heads, a.n_kv_heads, a.head_dim, a.scale = 2, 4, 4, 64, 0.125
    return a


def _need(a, n):
    return a.M * a.n_heads * n * (a.head_dim + 2) * 4


def _status(a, n_splits, ws, nbytes):
    l = _lib.lib()
    return l.licv_decode_attn_split(ctypes.byref(a), n_splits, ws, nbytes, None), l.licv_last_error()


def test_symbols_are_declared_and_exported_and_the_version_stays_9():
    l = _lib.lib()
    for name in ("licv_decode_attn_split_plan", "licv_decode_attn_split"):
        assert name in _lib.declared_symbols() and hasattr(l, name), name
    assert l.licv_decode_attn_split.argtypes == [ctypes.POINTER(_lib.DecodeAttnArgs), ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert l.licv_decode_attn_split_plan.restype is ctypes.c_int64
    assert _lib.check_exports()
    assert l.licv_version() == 9 == _lib.ABI_VERSION == _lib.header_abi_version()
    m = re.search(r"#define\s+LICV_DECODE_MAX_SPLITS\s+(\d+)", _lib.HEADER.read_text())
    assert m and int(m.group(1)) == _lib.DECODE_MAX_SPLITS == 32


@pytest.mark.parametrize("M,nh,nkv,hd", [(1, 32, 8, 128), (3, 4, 2, 128), (8, 32, 8, 128), (24, 32, 8, 128), (24, 32, 32, 128), (5, 4, 4, 96), (700, 4, 4, 64)])
def test_plan_is_deterministic_and_within_its_bounds(M, nh, nkv, hd):
    for Sk in (1, 37, 64, 65, 128, 129, 800, 2900, 10240, 10241, 12000, 20000, 1 << 20):
        n, nbytes = _plan(M, nh, nkv, hd, Sk)
        assert (n, nbytes) == _plan(M, nh, nkv, hd, Sk)
        assert 1 <= n <= min(32, -(-Sk // 64)), (M, nkv, Sk, n)
        if Sk <= 64:
            assert n == 1
        assert nbytes == M * nh * n * (hd + 2) * 4
    assert _lib.lib().licv_decode_attn_split_plan(M, nh, nkv, hd, 12000, None) == _plan(M, nh, nkv, hd, 12000)[1]   # n_splits may be NULL


def test_plan_splits_a_long_history_of_few_rows():
    n, _ = _plan(1, 32, 8, 128, 12000)
    assert n > 1


def test_bad_arguments_are_reported_not_crashed():
    l = _lib.lib()
    ws, big = 4096, 1 << 30
    assert l.licv_decode_attn_split(None, 0, ws, big, None) == -1 and b"null pointer" in l.licv_last_error()
    for field in ("qkv_bf16", "cos", "sin", "position_ids", "cache", "out"):
        a = _good()
        setattr(a, field, None)
        st, msg = _status(a, 0, ws, big)
        assert st == -1 and b"null pointer" in msg, field
    a = _good(); a.qkv_bf16 = None; a.qkv_ws = 4096; a.splits = 0                  # slices, badly described
    st, msg = _status(a, 0, ws, big)
    assert st == -1 and b"split-K workspace" in msg
    a = _good(); a.head_dim = 100
    st, msg = _status(a, 0, ws, big)
    assert st == -1 and b"head_dim 100" in msg
    a = _good(); a.past = a.max_len
    st, msg = _status(a, 0, ws, big)
    assert st == -1 and b"past" in msg
    st, msg = _status(_good(), 33, ws, big)
    assert st == -1 and b"n_splits 33" in msg and b"32" in msg
    a = _good()                                                                    # 201 keys: 4 sweeps, so 2 and 4 splits hold as asked
    st, msg = _status(a, 2, None, big)
    assert st == -1 and b"null workspace" in msg
    for n in (1, 2, 4):
        st, msg = _status(a, n, ws, _need(a, n) - 1)
        assert st == -1 and b"workspace of" in msg and str(_need(a, n)).encode() in msg, n
    st, msg = _status(a, 32, ws, _need(a, 4) - 1)                                  # 32 asked, clamped to the 4 sweeps
    assert st == -1 and b"workspace of" in msg and str(_need(a, 4)).encode() in msg and b"4 splits" in msg
    st, msg = _status(a, 2, ws + 8, big)
    assert st == -1 and b"16-byte aligned" in msg and b"workspace" in msg
    a = _good(); a.kv_rows = 4096; a.ld_kv_rows = 200
    st, msg = _status(a, 0, ws, big)
    assert st == -1 and b"kv_rows" in msg


def test_a_history_beyond_the_single_launch_limit_passes_the_argument_checks():
    l = _lib.lib()
    a = _good(past=19999)
    assert l.licv_decode_attn(ctypes.byref(a), None) == -1 and b"LDS budget" in l.licv_last_error()      # the single launch refuses it
    n, nbytes = _plan(a.M, a.n_heads, a.n_kv_heads, a.head_dim, 20000)
    st, msg = _status(a, 0, 4096, nbytes - 1)                                      # too small on purpose: the call returns before a launch
    assert st == -1 and b"workspace of" in msg and str(nbytes).encode() in msg
    assert b"history" not in msg and b"LDS" not in msg
