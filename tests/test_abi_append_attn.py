"""licv_append_attn at the ABI: the symbol is exported, header / binding / library agree on the struct and on LICV_APPEND_MAX_T, and
argument errors are reported on the host before any launch (no GPU needed: every call here must return before it reaches one)."""
import ctypes
import re

from licv import _lib


def _header():
    return _lib.HEADER.read_text()


def test_symbol_is_exported_and_declared():
    assert "licv_append_attn" in _lib.declared_symbols()
    l = _lib.lib()
    assert hasattr(l, "licv_append_attn")
    assert l.licv_append_attn.argtypes == [ctypes.POINTER(_lib.AppendAttnArgs), ctypes.c_void_p]
    assert _lib.check_exports()


def test_header_binding_and_library_agree():
    text = _header()
    m = re.search(r"#define\s+LICV_APPEND_MAX_T\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.APPEND_MAX_T == 32
    body = re.search(r"typedef struct \{([^}]*)\}\s*licv_append_attn_args;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.findall(r"(\w+)\s*$", first)[0])
        names += [re.findall(r"(\w+)\s*$", x)[0] for x in rest]
    assert names == [n for n, _ in _lib.AppendAttnArgs._fields_], "field order of licv_append_attn_args, header vs ctypes"
    ctype_of = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        want = ctypes.c_void_p if "*" in decl else ctype_of[decl.split()[0]]
        for n in re.findall(r"(\w+)\s*(?:,|$)", decl):
            assert dict(_lib.AppendAttnArgs._fields_)[n] is want, n
    # the library was compiled from the same header: a struct filled through the binding passes every check up to the first bad field
    a = _good()
    a.scale = 0.5
    a.head_dim = 100
    assert _lib.lib().licv_append_attn(ctypes.byref(a), None) == -1 and b"head_dim 100" in _lib.lib().licv_last_error()


def _good():
    a = _lib.AppendAttnArgs()
    a.qkv_bf16 = a.cos = a.sin = a.position_ids = a.cache = a.out = 4096          # never dereferenced on the host
    a.ldq, a.n_pos, a.max_len, a.past = 3 * 256, 64, 16, 5
    a.M, a.T, a.n_heads, a.n_kv_heads, a.head_dim, a.append = 2, 3, 4, 4, 64, 1
    return a


def _status(a):
    l = _lib.lib()
    return l.licv_append_attn(ctypes.byref(a), None), l.licv_last_error()


def test_bad_arguments_are_reported_not_crashed():
    l = _lib.lib()
    assert l.licv_append_attn(None, None) == -1 and b"null pointer" in l.licv_last_error()
    for field in ("qkv_bf16", "cos", "sin", "position_ids", "cache", "out"):
        a = _good()
        setattr(a, field, None)
        st, msg = _status(a)
        assert st == -1 and b"null pointer" in msg, field
    a = _good(); a.T = 0
    st, msg = _status(a)
    assert st == -1 and b"T = 0" in msg and b"32" in msg
    a = _good(); a.T = _lib.APPEND_MAX_T + 1; a.max_len = 64
    st, msg = _status(a)
    assert st == -1 and b"T = 33" in msg and b"32" in msg
    for hd in (4, 100, 136, 256):
        a = _good(); a.head_dim = hd; a.ldq = 3 * 4 * hd
        st, msg = _status(a)
        assert st == -1 and b"head_dim" in msg, hd
    a = _good(); a.past = 14                                                       # past + T beyond the cache row
    st, msg = _status(a)
    assert st == -1 and b"past" in msg
    a = _good(); a.n_kv_heads = 3
    assert _status(a)[0] == -1
    a = _good(); a.ldq = 100
    st, msg = _status(a)
    assert st == -1 and b"ldq" in msg
    a = _good(); a.append = 2
    st, msg = _status(a)
    assert st == -1 and b"append" in msg
    a = _good(); a.kv_rows = 4096; a.ld_kv_rows = 4
    st, msg = _status(a)
    assert st == -1 and b"kv_rows" in msg
