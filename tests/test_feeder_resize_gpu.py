"""ImageFeeder(resize=...): raw images of any size in, the resize on the side stream, the same pixel_values as preprocess_images on
the Pillow-resized batch; without `resize` the feeder is today's."""
import numpy as np
import pytest
import torch
from PIL import Image

import resample_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(40, 52), (165, 113), (100, 150), (64, 64), (17, 9), (131, 77)]      # (w, h)


def raw(i):
    w, h = SHAPES[i % len(SHAPES)]
    return RR.noise_image(w, h, seed=50 + i)


def test_five_batches_through_two_slots_bicubic():
    from licv import frontend
    from licv.image_feeder import ImageFeeder
    H = W = 64
    feeder = ImageFeeder(DEV, 6, H, W, resize="bicubic", max_src_bytes=6 * 165 * 150 * 3)
    batches = [[raw(6 * b + j) for j in range(3 + b % 3)] for b in range(5)]
    batches[2][1] = Image.fromarray(batches[2][1])                              # a PIL image is taken as it is
    want = []
    for imgs in batches:
        u8 = np.stack([np.asarray(Image.fromarray(np.asarray(im)).resize((W, H), resample=Image.BICUBIC)) for im in imgs])
        want.append(frontend.preprocess_images(torch.from_numpy(u8).to(DEV))[0])
    tickets, got = [], []
    tickets.append(feeder.submit(batches[0]))
    for b in range(5):
        if b + 1 < 5:
            tickets.append(feeder.submit(batches[b + 1]))                       # the next batch is queued while this one is read
        pv, m = feeder.get(tickets[b])
        assert m is None and pv.shape == (len(batches[b]), 3, H, W)
        got.append(pv.clone())
        feeder.release(tickets[b])
    for b in range(5):
        assert torch.equal(got[b], want[b]), f"batch {b}"


def test_ragged_targets_with_mask_bilinear():
    from licv import frontend
    from licv.image_feeder import ImageFeeder
    H, W = 98, 84
    feeder = ImageFeeder(DEV, 5, H, W, mean=frontend.IDEFICS2_MEAN, std=frontend.IDEFICS2_STD, with_mask=True, resize="bilinear")
    imgs = [raw(0), raw(1), None, raw(2), raw(3)]
    sizes = [(98, 70), (56, 84), None, (98, 84), None]                          # the last keeps its own 64 x 64
    padded = np.zeros((5, H, W, 3), np.uint8)
    hw = np.zeros((5, 2), np.int32)
    for i, (im, s) in enumerate(zip(imgs, sizes)):
        if im is None:
            continue
        r = im if s is None else np.asarray(Image.fromarray(im).resize((s[1], s[0]), resample=Image.BILINEAR))
        padded[i, :r.shape[0], :r.shape[1]] = r
        hw[i] = r.shape[:2]
    want, want_mask = frontend.preprocess_images(torch.from_numpy(padded).to(DEV), frontend.IDEFICS2_MEAN, frontend.IDEFICS2_STD,
                                                 valid_hw=torch.from_numpy(hw), want_mask=True)
    pv, m = feeder.get(feeder.submit(imgs, sizes))
    assert torch.equal(pv, want) and torch.equal(m, want_mask)


def test_feeder_without_resize_is_unchanged():
    from licv import frontend
    from licv.image_feeder import ImageFeeder
    H = W = 32
    feeder = ImageFeeder(DEV, 4, H, W, with_mask=True)
    assert feeder.resize is None and not hasattr(feeder, "stages") and feeder.host[0].is_pinned()
    u8 = np.random.default_rng(3).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    pv, m = feeder.get(feeder.submit(u8))
    want, want_mask = frontend.preprocess_images(torch.from_numpy(u8).to(DEV), want_mask=True)
    assert torch.equal(pv, want) and torch.equal(m, want_mask)
    ragged = [u8[0][:20, :17], None, u8[2]]
    pv, m = feeder.get(feeder.submit(ragged))
    padded = np.zeros((3, H, W, 3), np.uint8)
    padded[0, :20, :17] = ragged[0]
    padded[2] = u8[2]
    want, want_mask = frontend.preprocess_images(torch.from_numpy(padded).to(DEV), valid_hw=torch.tensor([[20, 17], [0, 0], [H, W]], dtype=torch.int32),
                                                 want_mask=True)
    assert torch.equal(pv, want) and torch.equal(m, want_mask)
    with pytest.raises(AssertionError):
        feeder.submit(u8, sizes=[(8, 8)] * 4)
