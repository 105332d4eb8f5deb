"""Device-side front-end of the hot path: the integer rules between the collator / processor and the first
GEMM as HIP kernels (csrc/frontend.hip), so that a forward pass makes no host round trip.

  * ``idefics_image_attention_mask`` — what ``processor.prepare_input`` hands the model as ``image_attention_mask``
    (ref:icv_src/icv_datamodule.py:80-124 -> hf:idefics/processing_idefics.py:89-133), from ``input_ids`` on the device;
  * ``idefics2_patch_front``         — padding-image flags, patch validity and NaViT position ids
    (hf:idefics2/modeling_idefics2.py:831-855, :136-170);
  * ``merge_image_rows_``            — Idefics2 ``inputs_merger`` (hf:idefics2/modeling_idefics2.py:789-815) without ``nonzero()``;
  * ``preprocess_images``            — uint8 -> normalised bf16 pixel_values (+ Idefics2's padding and mask);
  * ``resize_images``                — the resize (+ crop) in front of it, bit-equal to Pillow's ``Image.resize`` (csrc/resize.hip), from
    the host-side coefficient plans of ``resample_plan``.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import _p, _stream


def idefics_image_attention_mask(input_ids: torch.Tensor, image_token_id: int, eod_token_id: int, n_images: int,
                                 dtype: torch.dtype = torch.int32) -> torch.Tensor:
    """(B, S) int64 ids on the GPU -> (B, S, n_images) one-hot rows: token t attends the most recent <image> at or before t,
    nothing before the first image or between an end-of-document token and the next image.  int32 is what the engine's
    attention kernel reads; pass ``dtype=torch.long`` for the processor's own dtype."""
    assert input_ids.is_cuda and input_ids.dtype == torch.int64 and input_ids.dim() == 2
    ids = input_ids.contiguous()
    B, S = ids.shape
    out = torch.empty((B, S, n_images), dtype=torch.int32, device=ids.device)
    check(_lib.lib().licv_idefics_image_attention_mask(_p(ids), _p(out), B, S, n_images, int(image_token_id), int(eod_token_id), _stream(ids)))
    return out if dtype == torch.int32 else out.to(dtype)


_bounds: dict = {}


def navit_boundaries(n_side: int, device) -> torch.Tensor:
    """The fp32 bucket boundaries exactly as the HF module builds them (torch.arange on the host, uploaded once)."""
    key = (n_side, str(device))
    if key not in _bounds:
        _bounds[key] = torch.arange(1 / n_side, 1.0, 1 / n_side).to(device=device, dtype=torch.float32).contiguous()
    return _bounds[key]


def idefics2_patch_front(pixel_values: torch.Tensor, pixel_attention_mask: Optional[torch.Tensor], patch: int, n_side: int):
    """pixel_values (n, 3, H, W) bf16, pixel_attention_mask (n, H, W) bool or None ->
    (real (n,) int32, patch_valid (n, gh*gw) int32, position_ids (n, gh*gw) int64), all on the device."""
    assert pixel_values.is_cuda and pixel_values.dtype == torch.bfloat16 and pixel_values.is_contiguous() and pixel_values.dim() == 4
    n, _, H, W = pixel_values.shape
    gh, gw = H // patch, W // patch
    dev = pixel_values.device
    pam = None
    if pixel_attention_mask is not None:
        pam = pixel_attention_mask.to(device=dev, dtype=torch.bool).reshape(n, H, W).contiguous().view(torch.uint8)
    real = torch.empty((n,), dtype=torch.int32, device=dev)
    valid = torch.empty((n, gh * gw), dtype=torch.int32, device=dev)
    pos = torch.empty((n, gh * gw), dtype=torch.int64, device=dev)
    check(_lib.lib().licv_idefics2_patch_front(_p(pixel_values), _p(pam), _p(navit_boundaries(n_side, dev)), _p(real), _p(valid), _p(pos),
                                               n, H, W, patch, n_side, _stream(pixel_values)))
    return real, valid, pos


def merge_image_rows_(h: torch.Tensor, input_ids: torch.Tensor, image_rows: torch.Tensor, image_token_id: int) -> torch.Tensor:
    """In place: rows of h (M, dim) bf16 whose token is <image> take the image rows in order.  Returns the device-side count of
    <image> tokens (1-element int32 tensor; reading it is the caller's choice — it costs a sync)."""
    assert h.is_cuda and h.dtype == torch.bfloat16 and h.is_contiguous() and image_rows.dtype == torch.bfloat16 and image_rows.is_contiguous()
    ids = input_ids.reshape(-1).contiguous()
    M, dim = h.shape
    assert ids.numel() == M and ids.dtype == torch.int64
    scratch = torch.empty((M + 1,), dtype=torch.int32, device=h.device)
    check(_lib.lib().licv_merge_image_rows(_p(h), _p(ids), _p(image_rows), _p(scratch), C.c_void_p(scratch.data_ptr() + 4 * M), M, dim,
                                           image_rows.shape[0], int(image_token_id), _stream(h)))
    return scratch[M:]


# ------------------------------------------------------------------------------------------ image input (uint8 -> normalised bf16)
IDEFICS_MEAN = (0.48145466, 0.4578275, 0.40821073)        # hf:idefics/image_processing_idefics.py IDEFICS_STANDARD_MEAN / _STD
IDEFICS_STD = (0.26862954, 0.26130258, 0.27577711)
IDEFICS2_MEAN = IDEFICS2_STD = (0.5, 0.5, 0.5)              # hf:idefics2 image processor (IMAGENET_STANDARD_MEAN / _STD)


def preprocess_images(u8: torch.Tensor, mean=IDEFICS_MEAN, std=IDEFICS_STD, rescale: float = 1 / 255,
                      valid_hw: Optional[torch.Tensor] = None, want_mask: bool = False, out: Optional[torch.Tensor] = None,
                      mask_out: Optional[torch.Tensor] = None):
    """u8 (n, H, W, 3) uint8 on the GPU -> (pixel_values (n, 3, H, W) bf16, pixel_attention_mask (n, H, W) bool or None): the
    rescale + normalise + channels-first of the HF image processors (and, with `valid_hw` (n, 2) int32 = real height / width of each
    image inside its padded H x W, Idefics2's zero padding and mask), as one HIP kernel (csrc/frontend.hip).  The images arrive at their
    final size: resized on the host where the reference has it (in the dataset workers), or on the device by `resize_images`, which
    applies the same table to the bytes it resizes and so returns what this function returns on Pillow's bytes."""
    assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[-1] == 3 and u8.is_contiguous()
    n, H, W, _ = u8.shape
    dev = u8.device
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.bfloat16, device=dev)
    m = None
    if want_mask or mask_out is not None:
        m = mask_out if mask_out is not None else torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    hw = None
    if valid_hw is not None:
        hw = valid_hw.to(device=dev, dtype=torch.int32).contiguous()
        assert hw.shape == (n, 2)
    mean3, std3 = (C.c_float * 3)(*[float(x) for x in mean]), (C.c_float * 3)(*[float(x) for x in std])
    check(_lib.lib().licv_preprocess_images(_p(u8), _p(hw), _p(out), _p(m), n, H, W, C.c_double(float(rescale)), mean3, std3, _stream(u8)))
    return out, (m.view(torch.bool) if m is not None else None)


# ------------------------------------------------------------------------------------------ resize (bit-equal to Pillow's Image.resize)
_FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}
_PIL_FILTERS = {3: "bicubic", 2: "bilinear"}                  # PIL.Image.BICUBIC / BILINEAR
PRECISION_BITS = 22                                          # Pillow Resample.c: 32 - 8 - 2


def _filter_name(filter) -> str:
    name = _PIL_FILTERS.get(filter, filter)
    name = name.lower() if isinstance(name, str) else name
    if name not in _FILTER_SUPPORT:
        raise ValueError(f"resize filter {filter!r}: 'bicubic' or 'bilinear'")
    return name


def resample_plan(in_size: int, out_size: int, filter="bicubic"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for one axis, in IEEE double and in Pillow's
    order of operations -> (xmin int32[out_size], count int32[out_size], coef int32[out_size, ksize]): output index i reads the
    `count[i]` source indices from `xmin[i]` with the fixed-point (22 fractional bits) weights `coef[i, :count[i]]`; the rest of a
    row is 0.  Cached per (in_size, out_size, filter); the arrays are read-only.  Computed here and not on the device: a contracted
    multiply-add in the filter polynomial could move a coefficient by one."""
    return _resample_plan(int(in_size), int(out_size), _filter_name(filter))


@functools.lru_cache(maxsize=512)
def _resample_plan(in_size: int, out_size: int, name: str):
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_plan: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = _FILTER_SUPPORT[name] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    k = np.arange(ksize, dtype=np.int64)
    x = np.abs(((k[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    if name == "bicubic":
        a = -0.5
        w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    else:
        w = np.where(x < 1.0, 1.0 - x, 0.0)
    w[k[None, :] >= count[:, None]] = 0.0
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                   # a running sum from tap 0, as the C loop adds (np.sum adds pairwise)
        ww = ww + w[:, j]
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz][:, None]
    fixed = w * float(1 << PRECISION_BITS)
    coef = np.where(w < 0, np.trunc(-0.5 + fixed), np.trunc(0.5 + fixed)).astype(np.int32)
    out = (xmin.astype(np.int32), count.astype(np.int32), coef)
    for arr in out:
        arr.flags.writeable = False
    return out


def clip_resize_geometry(w: int, h: int, size: int):
    """hf CLIPImageProcessor's geometry for a w x h image: shortest edge -> `size` (the long edge is int(size * long / short)), then a
    centred size x size crop.  -> ((new_w, new_h), (left, top)).  The host path (resize_center_crop_u8) and the device path share it."""
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    return (nw, nh), ((nw - size) // 2, (nh - size) // 2)


_DESC_FIELDS = 16                                            # int64 fields of licv_resize_desc (include/licv_hip.h)


class ResizeStage:
    """One staging slot of the device resize: pinned host buffers (packed source bytes, descriptors, coefficient plans), their device
    copies and the workspace.  pack() fills the host side, launch() queues the copies and the two kernels on the current stream.
    Buffers grow on demand unless `fixed` (the feeder's slots: sized once)."""

    def __init__(self, device, src_bytes: int = 0, max_images: int = 0, fixed: bool = False):
        self.device = torch.device(device)
        self.fixed = fixed
        self.h_src = self.d_src = self.h_desc = self.d_desc = self.h_plan = self.d_plan = self.ws = None
        self.busy = None                                     # event: the last batch's copies and kernels have finished with the buffers
        self._grow_src(max(int(src_bytes), 1))
        self._grow_desc(max(int(max_images), 1))
        self._grow_plan(1 << 14)

    def _grow_src(self, nbytes):
        self.h_src = torch.empty((nbytes,), dtype=torch.uint8).pin_memory()
        self.d_src = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)

    def _grow_desc(self, n):
        self.h_desc = torch.zeros((n, _DESC_FIELDS), dtype=torch.int64).pin_memory()
        self.d_desc = torch.empty((n, _DESC_FIELDS), dtype=torch.int64, device=self.device)

    def _grow_plan(self, elems):
        self.h_plan = torch.empty((elems,), dtype=torch.int32).pin_memory()
        self.d_plan = torch.empty((elems,), dtype=torch.int32, device=self.device)

    def pack(self, images: Sequence, sizes, crops, filter) -> int:
        """images: (h, w, 3) uint8 arrays, PIL images (converted with .convert("RGB")) or None (a missing image); sizes: per image
        (out_h, out_w) or None (= the image's own size); crops: per image (top, left, height, width) inside the resized image or None
        (= all of it).  Returns n."""
        if self.busy is not None:
            self.busy.synchronize()                          # the previous batch has left the stage's buffers
            self.busy = None
        name = _filter_name(filter)
        n = len(images)
        arrs = []
        for im in images:
            if im is None:
                arrs.append(None)
                continue
            if not isinstance(im, np.ndarray):
                im = np.asarray(im.convert("RGB") if hasattr(im, "convert") else im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"resize: images are (h, w, 3) uint8, got {im.dtype} {im.shape}")
            arrs.append(im)
        total = sum(a.size for a in arrs if a is not None)
        if total > self.h_src.numel() or n > self.h_desc.shape[0]:
            if self.fixed:
                raise ValueError(f"resize: batch of {n} images / {total} source bytes exceeds the stage ({self.h_desc.shape[0]} images, "
                                 f"{self.h_src.numel()} bytes)")
            if total > self.h_src.numel():
                self._grow_src(max(total, 2 * self.h_src.numel()))
            if n > self.h_desc.shape[0]:
                self._grow_desc(max(n, 2 * self.h_desc.shape[0]))
        src, desc = self.h_src.numpy(), self.h_desc.numpy()
        plans, plan_off, plan_elems = [], {}, 0

        def plan(in_size, out_size):
            nonlocal plan_elems
            key = (in_size, out_size)
            if key not in plan_off:
                xmin, count, coef = resample_plan(in_size, out_size, name)
                plan_off[key] = (plan_elems, coef.shape[1])
                plans.extend((xmin, count, coef.reshape(-1)))
                plan_elems += 2 * out_size + coef.size
            return plan_off[key]

        off = 0
        for i, a in enumerate(arrs):
            desc[i] = 0
            if a is None or a.shape[0] == 0 or a.shape[1] == 0:
                continue
            h, w = a.shape[:2]
            oh, ow = (h, w) if sizes is None or sizes[i] is None else (int(sizes[i][0]), int(sizes[i][1]))
            top, left, ch, cw = (0, 0, oh, ow) if crops is None or crops[i] is None else (int(v) for v in crops[i])
            hp = plan(w, ow) if w != ow else (0, 0)
            vp = plan(h, oh) if h != oh else (0, 0)
            src[off:off + a.size] = a.reshape(-1)
            desc[i] = (off, 3 * w, 0, h, w, oh, ow, top, left, ch, cw, hp[0], hp[1], vp[0], vp[1], 0)
            off += a.size
        if plan_elems > self.h_plan.numel():
            self._grow_plan(max(plan_elems, 2 * self.h_plan.numel()))
        if plans:
            np.concatenate(plans, out=self.h_plan.numpy()[:plan_elems])
        self.n, self.src_bytes, self.plan_elems = n, off, plan_elems
        nb = C.c_int64(0)
        check(_lib.lib().licv_resize_images_workspace(C.c_void_p(self.h_desc.data_ptr()), n, C.byref(nb)))
        self.ws_bytes = nb.value
        return n

    def launch(self, H: int, W: int, out_u8=None, out_bf16=None, mask=None, mean=IDEFICS_MEAN, std=IDEFICS_STD, rescale: float = 1 / 255,
               upload: bool = True):
        """Queue H2D + the kernels for the packed batch on the current stream.  Argument errors raise before anything is written to
        the output.  upload=False runs the kernels again on the batch already on the device (measurements)."""
        n = self.n
        if self.ws is None or self.ws.numel() < self.ws_bytes:
            self.ws = torch.empty((max(self.ws_bytes, 16),), dtype=torch.uint8, device=self.device)
        try:
            if n and upload:
                self.d_src[:self.src_bytes].copy_(self.h_src[:self.src_bytes], non_blocking=True)
                self.d_desc[:n].copy_(self.h_desc[:n], non_blocking=True)
                self.d_plan[:self.plan_elems].copy_(self.h_plan[:self.plan_elems], non_blocking=True)
            mean3, std3 = (C.c_float * 3)(*[float(x) for x in mean]), (C.c_float * 3)(*[float(x) for x in std])
            check(_lib.lib().licv_resize_images(_p(self.d_src), self.src_bytes, C.c_void_p(self.h_desc.data_ptr()), _p(self.d_desc), n,
                                                _p(self.d_plan), self.plan_elems, H, W, _p(out_u8), _p(out_bf16), _p(mask),
                                                C.c_double(float(rescale)), mean3, std3, _p(self.ws), self.ws.numel(), _stream(self.d_src)))
        finally:
            self.busy = torch.cuda.Event()                   # the copies and the kernels have finished with the stage's buffers
            self.busy.record(torch.cuda.current_stream(self.device))


_stages: dict = {}


def resize_images(images: Sequence, sizes, crops, filter, out_hw, *, normalize=None, want_mask: bool = False, device="cuda",
                  out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None):
    """Resize (+ crop, + pad) a ragged batch on the device, bit-equal to PIL `Image.resize((out_w, out_h), filter)` on 8-bit RGB
    (csrc/resize.hip).  images: list of (h, w, 3) uint8 arrays / PIL images / None (a missing image: all padding); sizes[i] = (out_h,
    out_w) or None (no resize); crops[i] = (top, left, height, width) inside the resized image or None; filter "bicubic" /
    "bilinear"; out_hw = (H, W), the frame every crop is placed in at the origin (zeros outside).  Packing goes through pinned memory.
    normalize=None -> (n, H, W, 3) uint8; normalize=(mean, std) or (mean, std, rescale) -> (n, 3, H, W) bf16, what preprocess_images
    returns on the resized bytes.  With want_mask the result is (tensor, mask (n, H, W) bool)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    H, W = int(out_hw[0]), int(out_hw[1])
    st = _stages.get(dev)
    if st is None:
        st = _stages[dev] = ResizeStage(dev, 1 << 20, 64)
    with torch.cuda.device(dev):
        n = st.pack(images, sizes, crops, filter)
        m = None
        if want_mask or mask_out is not None:
            m = mask_out if mask_out is not None else torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        if normalize is None:
            res = out if out is not None else torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            st.launch(H, W, out_u8=res, mask=m)
        else:
            res = out if out is not None else torch.empty((n, 3, H, W), dtype=torch.bfloat16, device=dev)
            mean, std = normalize[0], normalize[1]
            st.launch(H, W, out_bf16=res, mask=m, mean=mean, std=std, rescale=normalize[2] if len(normalize) > 2 else 1 / 255)
    if m is not None:
        return res, m.view(torch.bool)
    return res
