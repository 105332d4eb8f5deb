"""The resize arithmetic on the host: tests/resample_ref.py (an independent restatement of Pillow's 8-bit resampler) equals
PIL.Image.resize bit for bit, and licv.frontend.resample_plan equals the restatement's coefficients exactly.  The GPU tests compare
the kernel against both, so a Pillow whose arithmetic differs shows here and not as a kernel failure."""
import numpy as np
import pytest
from PIL import Image

import resample_ref as RR

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
IMAGES = {"noise": RR.noise_image, "smooth": RR.smooth_image}


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1][0]}x{c[1][1]}")
def test_restatement_equals_pillow(case, kind, filter):
    (w, h), (ow, oh) = case
    img = IMAGES[kind](w, h, seed=w * 31 + h)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), resample=PIL_FILTER[filter]))
    got = RR.resize(img, ow, oh, filter)
    assert got.shape == want.shape == (oh, ow, 3)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1][0]}x{c[1][1]}")
def test_resample_plan_equals_the_restatements_coefficients(case, filter):
    from licv import frontend
    (w, h), (ow, oh) = case
    for in_size, out_size in ((w, ow), (h, oh)):
        got = frontend.resample_plan(in_size, out_size, filter)
        want = RR.plan_arrays(in_size, out_size, filter)
        for g, x in zip(got, want):
            assert g.dtype == np.int32 and g.shape == x.shape
            assert np.array_equal(g, x)
        assert not got[2].flags.writeable                                     # cached: shared between callers
    assert frontend.resample_plan(w, ow, filter)[0] is frontend.resample_plan(w, ow, PIL_FILTER[filter])[0]     # PIL's constants name the same plan


def test_grey_image_converted_to_rgb():
    rng = np.random.default_rng(5)
    grey = Image.fromarray(rng.integers(0, 256, (52, 40), dtype=np.uint8), mode="L")
    rgb = grey.convert("RGB")
    for filter in ("bicubic", "bilinear"):
        want = np.asarray(rgb.resize((64, 83), resample=PIL_FILTER[filter]))
        assert np.array_equal(RR.resize(np.asarray(rgb), 64, 83, filter), want)


def test_clip_geometry_and_restatement_equal_resize_center_crop_u8(golden):
    from icv_src.utils.mm_topk_retriver import resize_center_crop_u8
    from licv import frontend
    g = golden("g18_clip_tiny")
    size = int(g["proc_size"])
    assert int(g["n_images"]) == 5
    for i in range(5):
        pil = Image.fromarray(g[f"img_{i}"])
        img = np.asarray(pil.convert("RGB"))                                   # the fixture holds an L image too
        h, w = img.shape[:2]
        (nw, nh), (left, top) = frontend.clip_resize_geometry(w, h, size)
        assert min(nw, nh) == size
        got = RR.resize(img, nw, nh, "bicubic")[top:top + size, left:left + size]
        assert np.array_equal(got, resize_center_crop_u8(pil, size))


def test_clip_geometry_rule():
    from licv.frontend import clip_resize_geometry
    assert clip_resize_geometry(640, 480, 224) == ((298, 224), (37, 0))
    assert clip_resize_geometry(480, 640, 224) == ((224, 298), (0, 37))
    assert clip_resize_geometry(165, 113, 64) == ((93, 64), (14, 0))
    assert clip_resize_geometry(224, 224, 224) == ((224, 224), (0, 0))
