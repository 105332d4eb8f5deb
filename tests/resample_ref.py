"""An independent restatement of Pillow's 8-bit resampler (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc) for the resize tests.  It shares no code with `licv`: the coefficients
are computed one output index and one tap at a time in Python floats (IEEE double), and the passes loop over output index and tap
(numpy only carries the other axis and the three channels, in int32 as the C accumulator)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}


def coefficients(in_size, out_size, filter):
    """-> (bounds [(xmin, count)] * out_size, coef: out_size lists of ksize ints)."""
    f, support = FILTERS[filter]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, coef = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)               # int() truncates, as the C cast
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * ss)
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        bounds.append((xmin, xmax))
        coef.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
    return bounds, coef


def plan_arrays(in_size, out_size, filter):
    """The same as three int32 arrays (xmin, count, coef[out_size, ksize])."""
    bounds, coef = coefficients(in_size, out_size, filter)
    return (np.array([b[0] for b in bounds], dtype=np.int32), np.array([b[1] for b in bounds], dtype=np.int32), np.array(coef, dtype=np.int32))


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass_axis1(img, out_size, filter):
    """Resample axis 1 of (rows, in_size, 3) uint8."""
    bounds, coef = coefficients(img.shape[1], out_size, filter)
    src = img.astype(np.int32)
    out = np.empty((img.shape[0], out_size, 3), dtype=np.uint8)
    for xx in range(out_size):
        xmin, count = bounds[xx]
        acc = np.full((img.shape[0], 3), 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for x in range(count):
            acc += src[:, xmin + x, :] * np.int32(coef[xx][x])
        out[:, xx, :] = _clip8(acc)
    return out


def resize(img, out_w, out_h, filter):
    """(h, w, 3) uint8 -> (out_h, out_w, 3) uint8 as PIL's Image.resize((out_w, out_h), filter): horizontal pass, rounded to uint8,
    then vertical pass; a pass runs only if its axis changes size."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    if out_w != w:
        img = _pass_axis1(img, out_w, filter)
    if out_h != h:
        img = _pass_axis1(img.transpose(1, 0, 2), out_h, filter).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


# the (w, h) -> (ow, oh) cases of the resize tests, and their two kinds of image
CASES = [((1, 7), (5, 3)), ((17, 9), (224, 224)), ((40, 52), (64, 83)), ((165, 113), (93, 64)), ((100, 150), (64, 96)),
         ((224, 224), (224, 100)), ((640, 480), (298, 224)), ((1024, 768), (224, 224))]


def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_image(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = []
    for _ in range(3):
        f, ph = rng.uniform(0.5, 3.0, 2), rng.uniform(0, 6.28, 2)
        ch.append(128 + 120 * np.sin(2 * np.pi * f[0] * xx / max(w, 2) + ph[0]) * np.cos(2 * np.pi * f[1] * yy / max(h, 2) + ph[1]))
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
