"""ABI 9: the device resize is exported and header, library and binding agree on the version (no GPU needed)."""
import ctypes as C

import numpy as np


def test_resize_exports_and_version_9():
    from licv import _lib
    assert _lib.check_exports()
    assert _lib.lib().licv_version() == _lib.ABI_VERSION == _lib.header_abi_version() == 9
    for name in ("licv_resize_images", "licv_resize_images_workspace"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)


def test_workspace_query_lays_out_the_horizontal_rows_and_checks_the_crop():
    """Host-only part of the entry point: offsets are the running sum of h * align16(3 cw) over the images with a horizontal pass."""
    from licv import _lib
    d = np.zeros((4, 16), dtype=np.int64)
    #        off ld        x0 h    w    oh   ow   top left ch   cw   hp hk vp vk ws
    d[0] = (0, 3 * 640, 0, 480, 640, 224, 298, 0, 37, 224, 224, 0, 11, 0, 11, -1)
    d[1] = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1)                              # a missing image
    d[2] = (0, 3 * 224, 0, 224, 224, 100, 224, 0, 0, 100, 224, 0, 0, 0, 5, -1)            # vertical pass only
    d[3] = (0, 3 * 17, 0, 9, 17, 224, 224, 0, 0, 224, 5, 0, 5, 0, 5, -1)
    nb = C.c_int64(-7)
    assert _lib.lib().licv_resize_images_workspace(C.c_void_p(d.ctypes.data), 4, C.byref(nb)) == 0
    assert d[:, 15].tolist() == [0, 480 * 672, 480 * 672, 480 * 672] and nb.value == 480 * 672 + 9 * 16
    d[3, 8] = 220                                                                          # left + cw > ow
    nb = C.c_int64(-7)
    assert _lib.lib().licv_resize_images_workspace(C.c_void_p(d.ctypes.data), 4, C.byref(nb)) == -1 and nb.value == -7
    assert b"image 3" in _lib.lib().licv_last_error() and b"outside the resized image" in _lib.lib().licv_last_error()
