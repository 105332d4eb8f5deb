"""MMTopkRetriever with device_resize: the images' raw bytes go to the device and licv_resize_images does what the PIL thread pool +
licv_preprocess_images do on the host path - the same bytes, so the same features bit for bit and the same retrieve() lists."""
import numpy as np
import pytest
import torch
from PIL import Image

from test_retriever_gpu import N_INDEX, SOURCES, pattern, perturbed, tower

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(241, 257), (333, 251), (229, 401), (640, 480), (225, 227), (517, 389)]      # (w, h): odd, both orientations, above the crop size


def datasets():
    index_u8 = [pattern(100 + i, *SIZES[i % len(SIZES)]) for i in range(N_INDEX)]
    test_u8 = [perturbed(index_u8[s], 200 + j) for j, s in enumerate(SOURCES)]
    train_ds = [dict(image=Image.fromarray(a)) for a in index_u8]
    val_ds = [dict(image=Image.fromarray(a)) for a in test_u8]
    val_ds[1]["image"] = val_ds[1]["image"].convert("L")                      # converted to RGB on the host, as today
    return train_ds, val_ds


def build(M, train_ds, val_ds, weights):
    return M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, index_field="image", mode="i2i", batch_size=8, num_workers=4,
                             cache_file=None, device=DEV, clip_weights=weights)


def test_device_resize_gives_the_host_paths_features_and_lists(monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    from licv import frontend
    weights = tower()
    train_ds, val_ds = datasets()
    assert M.MMTopkRetriever.device_resize is False

    host_calls, dev_calls = [], []                                           # list.append: the host path runs in worker threads
    host_crop, dev_resize = M.resize_center_crop_u8, frontend.resize_images
    monkeypatch.setattr(M, "resize_center_crop_u8", lambda *a, **k: (host_calls.append(1), host_crop(*a, **k))[1])
    monkeypatch.setattr(frontend, "resize_images", lambda *a, **k: (dev_calls.append(1), dev_resize(*a, **k))[1])

    host = build(M, train_ds, val_ds, weights)                               # the attribute at its default: the thread-pool path
    assert (len(host_calls), len(dev_calls)) == (N_INDEX + len(SOURCES), 0)

    monkeypatch.setattr(M.MMTopkRetriever, "device_resize", True)
    dev = build(M, train_ds, val_ds, weights)
    assert (len(host_calls), len(dev_calls)) == (N_INDEX + len(SOURCES), N_INDEX // 8 + 1)
    assert torch.equal(dev._index_dev, host._index_dev) and torch.equal(dev._test_dev, host._test_dev)
    assert np.array_equal(dev.index_features, host.index_features) and np.array_equal(dev.test_features, host.test_features)
    assert dev.retrieve(4) == host.retrieve(4) and dev.retrieve(1) == host.retrieve(1)


def test_pixel_values_of_both_paths_are_equal():
    """The step in front of the tower on its own, so a difference names the image."""
    import types
    from icv_src.utils import mm_topk_retriver as M
    arch, _ = tower()
    train_ds, _ = datasets()
    images = [d["image"] for d in train_ds[:len(SIZES)]]
    r = object.__new__(M.MMTopkRetriever)
    r._img_processor, r.device, r.vision_encoder = None, DEV, types.SimpleNamespace(arch=arch)
    host = r._pixel_values(images, None)
    r.device_resize = True
    dev = r._pixel_values(images, None)
    for i in range(len(images)):
        assert torch.equal(dev[i], host[i]), f"image {i} ({SIZES[i]})"
