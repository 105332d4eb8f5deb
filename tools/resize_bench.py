"""Image resize measurements: the CLIP front-end of RICE - 640 x 480 RGB -> shortest edge 224 (bicubic) -> centre crop
224 x 224 -> normalised bf16 - on the host path (PIL in a thread pool + licv_preprocess_images) beside the device path
(licv_resize_images), on one GPU in one process.  One JSON line per run, appended to profiles/resize_bench.jsonl.

  python tools/resize_bench.py [--out profiles/resize_bench.jsonl] [--batch 256] [--reps 20] [--workers 16]

Host and device paths: wall clock around work that ends in a device synchronise, alternating, median of --reps after warm-up.  Kernel
time: device events around the two launches on a batch already on the device, beside a device-to-device copy that moves the same
number of bytes.  The bytes are those the algorithm needs, computed from the shapes and the plans."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "licv-vqa_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

W_SRC, H_SRC, SIZE = 640, 480, 224


def photo_like(seed):
    """Smooth structure + noise: neither a flat image nor white noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H_SRC, 0:W_SRC]
    ch = [128 + 90 * np.sin(2 * np.pi * rng.uniform(0.5, 4) * xx / W_SRC + rng.uniform(0, 6)) * np.cos(2 * np.pi * rng.uniform(0.5, 4) * yy / H_SRC)
          for _ in range(3)]
    return np.clip(np.stack(ch, -1) + rng.normal(0, 12, (H_SRC, W_SRC, 3)), 0, 255).astype(np.uint8)


def wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return s


def events(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resize_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resize_bench measures on the GPU"
    from PIL import Image
    from icv_src.utils.mm_topk_retriver import CLIP_MEAN, CLIP_STD, resize_center_crop_u8
    from licv import frontend
    dev = torch.device("cuda:0")
    n = a.batch
    distinct = [photo_like(s) for s in range(8)]
    images = [Image.fromarray(distinct[i % 8].copy()) for i in range(n)]
    (nw, nh), (left, top) = frontend.clip_resize_geometry(W_SRC, H_SRC, SIZE)
    sizes, crops = [(nh, nw)] * n, [(top, left, SIZE, SIZE)] * n
    pool = ThreadPoolExecutor(a.workers)

    def host_path():
        u8 = np.stack(list(pool.map(lambda im: resize_center_crop_u8(im, SIZE), images)))
        return frontend.preprocess_images(torch.from_numpy(u8).to(dev), mean=CLIP_MEAN, std=CLIP_STD)[0]

    def device_path():
        rgb = [np.asarray(im.convert("RGB")) for im in images]
        return frontend.resize_images(rgb, sizes, crops, "bicubic", (SIZE, SIZE), normalize=(CLIP_MEAN, CLIP_STD), device=dev)

    same = bool(torch.equal(host_path(), device_path()))
    t_host, t_dev = [], []
    for _ in range(a.reps):                                  # alternating: both see the same neighbours on the host
        t_host += wall(host_path, 1, warmup=0)
        t_dev += wall(device_path, 1, warmup=0)
    t_host, t_dev = t_host[2:], t_dev[2:]                    # the first two rounds are warm-up
    t_pack = wall(lambda: frontend._stages[dev].pack([np.asarray(im.convert("RGB")) for im in images], sizes, crops, "bicubic"), max(3, a.reps // 4))

    # kernels alone, on the batch the last device_path() left on the device
    st = frontend._stages[dev]
    out = torch.empty((n, 3, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
    k_ms = events(lambda: st.launch(SIZE, SIZE, out_bf16=out, mean=CLIP_MEAN, std=CLIP_STD, upload=False), 5 * a.reps)
    xmin, count, _ = frontend.resample_plan(W_SRC, nw, "bicubic")
    cols = int(xmin[left + SIZE - 1] + count[left + SIZE - 1] - xmin[left])           # source columns the kept output columns read
    row_ws = (3 * SIZE + 15) // 16 * 16
    nbytes = n * (H_SRC * cols * 3 + 2 * H_SRC * row_ws + 3 * SIZE * SIZE * 2)        # source read + workspace write and read + bf16 written
    a_buf, b_buf = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    c_ms = events(lambda: b_buf.copy_(a_buf), 5 * a.reps)
    h2d = torch.empty(n * H_SRC * W_SRC * 3, dtype=torch.uint8).pin_memory()
    d_buf = torch.empty_like(h2d, device=dev)
    h_ms = events(lambda: d_buf.copy_(h2d, non_blocking=True), a.reps)

    med = statistics.median
    rec = dict(bench="resize", workload=f"{W_SRC}x{H_SRC} -> {nw}x{nh} bicubic -> crop {SIZE}x{SIZE} -> bf16 (CLIP)", batch=n, reps=len(t_host),
               workers=a.workers, outputs_bit_equal=same,
               host_images_per_s=round(n / med(t_host), 1), host_ms=round(med(t_host) * 1e3, 2), host_ms_min=round(min(t_host) * 1e3, 2),
               host_ms_max=round(max(t_host) * 1e3, 2),
               device_images_per_s=round(n / med(t_dev), 1), device_ms=round(med(t_dev) * 1e3, 2), device_ms_min=round(min(t_dev) * 1e3, 2),
               device_ms_max=round(max(t_dev) * 1e3, 2), device_pack_only_ms=round(med(t_pack) * 1e3, 2),
               h2d_raw_frames_ms=round(med(h_ms), 3), h2d_gb_per_s=round(h2d.numel() / med(h_ms) / 1e6, 1),
               kernels_ms=round(med(k_ms), 4), kernels_ms_min=round(min(k_ms), 4), kernels_ms_max=round(max(k_ms), 4),
               kernels_images_per_s=round(n / med(k_ms) * 1e3, 1), algorithm_bytes=nbytes, kernels_gb_per_s=round(nbytes / med(k_ms) / 1e6, 1),
               device_copy_same_bytes_ms=round(med(c_ms), 4), device_copy_gb_per_s=round(nbytes / med(c_ms) / 1e6, 1))
    print(json.dumps(rec), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()
