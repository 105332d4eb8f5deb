"""The retrieval entry points at the C-ABI: header, binding and library agree on ABI 8 and export the new symbols, and bad arguments
come back as LICV_E_BADARG before anything touches a device."""
import ctypes as C

from licv import _lib

NEW = ["licv_topk_ip", "licv_topk_ip_workspace", "licv_l2_normalize_rows", "licv_quick_gelu"]


def test_abi_8_exports_the_retrieval_symbols():
    assert _lib.check_exports()
    assert _lib.lib().licv_version() == _lib.ABI_VERSION == _lib.header_abi_version()
    assert _lib.ABI_VERSION >= 8
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(_lib.lib(), n), n


def _topk(Q, N, D, k, ws_bytes, ldq=None, ldx=None):
    l = _lib.lib()
    p = C.c_void_p(4096)                                    # never dereferenced: every case below is refused on the host
    st = l.licv_topk_ip(p, D if ldq is None else ldq, p, D if ldx is None else ldx, Q, N, D, k, p, p, p, ws_bytes, None)
    return st, l.licv_last_error().decode()


def test_topk_ip_refuses_bad_arguments_on_the_host():
    big = 1 << 40
    for Q, N, D, k, word in [(4, 100, 32, 0, "k = 0"), (4, 100, 32, 65, "k = 65"), (4, 10, 32, 11, "exceeds N"), (4, 100, 30, 4, "multiple of 4"),
                             (4, 100, 2048, 4, "multiple of 4"), (0, 100, 32, 4, "Q = 0"), (4, 1 << 31, 32, 4, "N = ")]:
        st, msg = _topk(Q, N, D, k, big)
        assert st == -1 and word in msg, (Q, N, D, k, st, msg)
        nb = C.c_int64(-7)
        assert _lib.lib().licv_topk_ip_workspace(Q, N, D, k, C.byref(nb)) == -1 and nb.value == -7
    st, msg = _topk(4, 100, 32, 4, big, ldq=30)
    assert st == -1 and "ldq" in msg
    nb = C.c_int64(0)
    assert _lib.lib().licv_topk_ip_workspace(300, 100000, 512, 32, C.byref(nb)) == 0
    assert nb.value > 0 and nb.value % (300 * 32 * 8) == 0 and nb.value <= 300 * 32 * 8 * 128      # Q * chunks * k entries of 8 bytes
    st, msg = _topk(300, 100000, 512, 32, nb.value - 1)
    assert st == -1 and "workspace" in msg
    st, msg = _lib.lib().licv_topk_ip(None, 32, None, 32, 4, 100, 32, 4, None, None, None, big, None), _lib.lib().licv_last_error().decode()
    assert st == -1 and "null pointer" in msg


def test_row_kernels_refuse_bad_arguments_on_the_host():
    l = _lib.lib()
    p = C.c_void_p(4096)
    assert l.licv_l2_normalize_rows(None, 0, None, 4, 8, None) == -1 and b"null pointer" in l.licv_last_error()
    assert l.licv_l2_normalize_rows(p, 5, p, 4, 8, None) == -1 and b"dtype" in l.licv_last_error()
    assert l.licv_l2_normalize_rows(p, 0, p, 0, 8, None) == -1 and b"bad shape" in l.licv_last_error()
    assert l.licv_quick_gelu(None, 4, 8, 8, None) == -1 and b"null pointer" in l.licv_last_error()
    assert l.licv_quick_gelu(p, 4, 8, 6, None) == -1 and b"bad shape" in l.licv_last_error()
