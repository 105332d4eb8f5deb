"""licv_resize_images on the GPU: the kernel's bytes equal Pillow's Image.resize (and tests/resample_ref.py, whose equality with Pillow
tests/test_resample_ref_cpu.py holds on the same inputs) bit for bit; the bf16 form equals preprocess_images on Pillow's bytes."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import resample_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
FILTERS = ["bicubic", "bilinear"]
CASE_IDS = [f"{c[0][0]}x{c[0][1]}->{c[1][0]}x{c[1][1]}" for c in RR.CASES]


@functools.lru_cache(maxsize=None)
def source(case_index, kind):
    (w, h), _ = RR.CASES[case_index]
    img = (RR.noise_image if kind == "noise" else RR.smooth_image)(w, h, seed=w * 31 + h)
    img.flags.writeable = False
    return img


@functools.lru_cache(maxsize=None)
def references(case_index, kind, filter):
    """(Pillow's bytes, the restatement's bytes) of a case: computed once, shared, read-only."""
    _, (ow, oh) = RR.CASES[case_index]
    img = source(case_index, kind)
    pil = np.asarray(Image.fromarray(img).resize((ow, oh), resample=PIL_FILTER[filter]))
    ref = RR.resize(img, ow, oh, filter)
    pil.flags.writeable = False
    ref.flags.writeable = False
    return pil, ref


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("ci", range(len(RR.CASES)), ids=CASE_IDS)
def test_one_image_per_call_equals_pillow(ci, kind, filter):
    from licv import frontend
    _, (ow, oh) = RR.CASES[ci]
    pil, ref = references(ci, kind, filter)
    got = frontend.resize_images([source(ci, kind)], [(oh, ow)], None, filter, (oh, ow), device=DEV)
    assert got.shape == (1, oh, ow, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got[0].cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(got, pil)


@pytest.mark.parametrize("filter", FILTERS)
def test_ragged_batch_with_a_missing_image_and_one_that_needs_no_resize(filter):
    from licv import frontend
    plain = RR.noise_image(61, 47, seed=9)                                   # goes through unchanged
    images = [source(i, "noise") for i in range(len(RR.CASES))]
    sizes = [(c[1][1], c[1][0]) for c in RR.CASES]
    images[3:3] = [None]
    sizes[3:3] = [None]
    images.append(plain)
    sizes.append(None)
    for (H, W) in ((224, 300), (225, 299)):                                  # 3 W a multiple of 4 (dword stores) and not
        got, mask = frontend.resize_images(images, sizes, None, filter, (H, W), want_mask=True, device=DEV)
        got, mask = got.cpu().numpy(), mask.cpu().numpy()
        assert got.shape == (len(images), H, W, 3) and mask.shape == (len(images), H, W) and mask.dtype == np.bool_
        refs = [references(i, "noise", filter) for i in range(len(RR.CASES))]
        refs[3:3] = [(np.zeros((0, 0, 3), np.uint8),) * 2]
        refs.append((plain, plain))
        for i, (pil, ref) in enumerate(refs):
            oh, ow = pil.shape[:2]
            want = np.zeros((H, W, 3), np.uint8)
            want[:oh, :ow] = pil
            want_mask = np.zeros((H, W), np.bool_)
            want_mask[:oh, :ow] = True
            assert np.array_equal(ref, pil)
            assert np.array_equal(got[i], want), f"image {i}"
            assert np.array_equal(mask[i], want_mask), f"mask {i}"


@pytest.mark.parametrize("w,h,size", [(640, 480, 224), (165, 113, 64), (113, 165, 64)])
def test_centre_crop_equals_resize_center_crop_u8(w, h, size):
    from icv_src.utils.mm_topk_retriver import resize_center_crop_u8
    from licv import frontend
    img = RR.noise_image(w, h, seed=w + h)
    (nw, nh), (left, top) = frontend.clip_resize_geometry(w, h, size)
    got = frontend.resize_images([img], [(nh, nw)], [(top, left, size, size)], "bicubic", (size, size), device=DEV)[0].cpu().numpy()
    assert np.array_equal(got, resize_center_crop_u8(Image.fromarray(img), size))
    assert np.array_equal(got, RR.resize(img, nw, nh, "bicubic")[top:top + size, left:left + size])


@pytest.mark.parametrize("constants", ["clip", "idefics", "idefics2"])
def test_bf16_form_equals_preprocess_images_of_pillows_bytes(constants):
    from icv_src.utils.mm_topk_retriver import CLIP_MEAN, CLIP_STD
    from licv import frontend
    mean, std = {"clip": (CLIP_MEAN, CLIP_STD), "idefics": (frontend.IDEFICS_MEAN, frontend.IDEFICS_STD),
                 "idefics2": (frontend.IDEFICS2_MEAN, frontend.IDEFICS2_STD)}[constants]
    cases = [2, 3, 4, 6]                                                     # 64x83, 93x64, 64x96, 298x224 inside a 224 x 300 frame
    H, W = 224, 300
    images = [source(i, "smooth") for i in cases] + [None]
    sizes = [(RR.CASES[i][1][1], RR.CASES[i][1][0]) for i in cases] + [None]
    padded = np.zeros((len(images), H, W, 3), np.uint8)
    hw = np.zeros((len(images), 2), np.int32)
    for j, i in enumerate(cases):
        pil = references(i, "smooth", "bicubic")[0]
        padded[j, :pil.shape[0], :pil.shape[1]] = pil
        hw[j] = pil.shape[:2]
    want, want_mask = frontend.preprocess_images(torch.from_numpy(padded).to(DEV), mean, std, valid_hw=torch.from_numpy(hw), want_mask=True)
    got, mask = frontend.resize_images(images, sizes, None, "bicubic", (H, W), normalize=(mean, std), want_mask=True, device=DEV)
    assert got.dtype == torch.bfloat16 and got.shape == (len(images), 3, H, W)
    assert torch.equal(got, want) and torch.equal(mask, want_mask)
    assert not got[-1].any() and not mask[-1].any() and not got[0, :, 83:].any() and not got[0, :, :, 64:].any()
    # without padding: the whole frame real, no mask asked for
    i = 6
    pil = references(i, "smooth", "bicubic")[0]
    want = frontend.preprocess_images(torch.from_numpy(pil[None].copy()).to(DEV), mean, std)[0]
    got = frontend.resize_images([source(i, "smooth")], [pil.shape[:2]], None, "bicubic", pil.shape[:2], normalize=(mean, std), device=DEV)
    assert torch.equal(got, want)


def test_image_that_needs_nothing_equals_preprocess_images():
    from licv import frontend
    img = RR.noise_image(37, 29, seed=2)
    want = frontend.preprocess_images(torch.from_numpy(img[None]).to(DEV))[0]
    got = frontend.resize_images([img], None, None, "bicubic", (29, 37), normalize=(frontend.IDEFICS_MEAN, frontend.IDEFICS_STD), device=DEV)
    assert torch.equal(got, want)
    assert np.array_equal(frontend.resize_images([img], [None], [None], "bilinear", (29, 37), device=DEV)[0].cpu().numpy(), img)


def test_source_window_of_a_larger_frame():
    """src_ld_bytes / x0_bytes: the source is a window of a wider frame (rows not tight, column 0 at an odd byte offset)."""
    import ctypes as C
    from licv import frontend
    frame = RR.noise_image(97, 71, seed=4)
    y0, x0, h, w, oh, ow = 5, 11, 52, 40, 83, 64
    sub = np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w])
    st = frontend.ResizeStage(DEV, frame.size, 1)
    st.pack([sub], [(oh, ow)], None, "bicubic")
    st.h_src.numpy()[:frame.size] = frame.reshape(-1)
    d = st.h_desc.numpy()[0]
    d[0], d[1], d[2] = y0 * frame.shape[1] * 3, frame.shape[1] * 3, 3 * x0
    st.src_bytes = frame.size
    out = torch.empty((1, oh, ow, 3), dtype=torch.uint8, device=DEV)
    st.launch(oh, ow, out_u8=out)
    assert np.array_equal(out[0].cpu().numpy(), np.asarray(Image.fromarray(sub).resize((ow, oh), resample=Image.BICUBIC)))


@pytest.mark.parametrize("what", ["crop outside the resized image", "frame smaller than the crop"])
def test_bad_geometry_is_an_error_and_writes_nothing(what):
    from licv import frontend
    from licv._lib import LicvError
    img = RR.noise_image(40, 52, seed=1)
    if what == "crop outside the resized image":
        crop, frame, text = (30, 0, 64, 64), (64, 64), "outside the resized image"      # top 30 + 64 rows > 83
    else:
        crop, frame, text = (0, 0, 83, 64), (64, 64), "larger than the frame"
    out = torch.full((1, frame[0], frame[1], 3), 77, dtype=torch.uint8, device=DEV)
    mask = torch.full((1, frame[0], frame[1]), 5, dtype=torch.uint8, device=DEV)
    with pytest.raises(LicvError, match=text):
        frontend.resize_images([img], [(83, 64)], [crop], "bicubic", frame, out=out, mask_out=mask, device=DEV)
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((mask == 5).all())
    good = frontend.resize_images([img], [(83, 64)], [(10, 0, 64, 64)], "bicubic", frame, device=DEV)      # the stage is usable afterwards
    assert np.array_equal(good[0].cpu().numpy(), np.asarray(Image.fromarray(img).resize((64, 83), resample=Image.BICUBIC))[10:74])
