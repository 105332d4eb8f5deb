"""RICE retrieval measurements: the fused exact search beside its unfused torch form, and the CLIP tower beside the
unfused PyTorch-ROCm restatement, on one GPU in one process.  One JSON line per shape, appended to profiles/retrieval_bench.jsonl.

  python tools/retrieval_bench.py [--out profiles/retrieval_bench.jsonl] [--reps 20] [--only topk|tower] [--one-batch]

Device-event timing, warm-up, median of --reps.  --one-batch runs a single tower batch and nothing else (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "licv-vqa_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FP32_MFMA_PEAK = 157.3e12            # MI355X, v_mfma_f32_32x32x2_f32
TOPK_SHAPES = [("vqav2", 5000, 443757, 512, 32), ("okvqa", 500, 9009, 512, 32)]


def timed(fn, reps, warmup=3):
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
    return statistics.median(ms), min(ms), max(ms)


def unit_rows(n, d, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    mean = torch.randn(d, generator=g, device=dev)
    mean /= mean.norm()
    x = mean + 0.7 * torch.randn(n, d, generator=g, device=dev) / d ** 0.5
    return (x / x.norm(dim=-1, keepdim=True)).contiguous()


def bench_topk(reps, out):
    import ctypes as C
    from licv import _lib, ops
    dev = torch.device("cuda:0")
    for name, Q, N, D, k in TOPK_SHAPES:
        q, x = unit_rows(Q, D, 1, dev), unit_rows(N, D, 2, dev)
        q_chunk = max(1, min(Q, (2 << 30) // (4 * N)))              # the unfused form's score matrix: at most 2 GiB at a time

        def unfused():
            idx = []
            for q0 in range(0, Q, q_chunk):
                idx.append(torch.topk(q[q0:q0 + q_chunk] @ x.T, k, dim=1))
            return idx

        fused = lambda: ops.topk_ip(q, x, k)
        i_f, s_f = fused()
        ref = unfused()
        i_u, s_u = torch.cat([r.indices for r in ref]), torch.cat([r.values for r in ref])
        same = float((i_f == i_u).float().mean())
        t_f, t_u = timed(fused, reps), timed(unfused, reps)
        nb = C.c_int64(0)
        _lib.check(_lib.lib().licv_topk_ip_workspace(Q, N, D, k, C.byref(nb)))
        flops = 2.0 * Q * N * D
        rec = dict(bench="topk_ip", shape=name, Q=Q, N=N, D=D, k=k, reps=reps,
                   fused_ms=round(t_f[0], 3), fused_ms_min=round(t_f[1], 3), fused_ms_max=round(t_f[2], 3),
                   unfused_ms=round(t_u[0], 3), unfused_ms_min=round(t_u[1], 3), unfused_ms_max=round(t_u[2], 3),
                   fused_tflops=round(flops / t_f[0] / 1e9, 2), unfused_tflops=round(flops / t_u[0] / 1e9, 2),
                   fused_share_of_fp32_mfma_peak=round(flops / (t_f[0] * 1e-3) / FP32_MFMA_PEAK, 4),
                   fused_bytes_written=int(nb.value + Q * k * 12), unfused_bytes_written=int(4 * Q * N + Q * k * 12),
                   unfused_q_chunk=q_chunk, index_positions_equal_to_unfused=round(same, 6),
                   max_score_difference=float((s_f - s_u).abs().max()))
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        del q, x


def bench_tower(reps, out, one_batch=False):
    import clip_ref as R
    from licv.clip_engine import ClipVisionEngine
    from licv.config import CLIP_VIT_B32 as arch
    from licv.synthetic import synth_clip_vision_weights, trained_like_
    dev = torch.device("cuda:0")
    n = 256
    sd = trained_like_(synth_clip_vision_weights(arch, seed=21, dtype=torch.bfloat16), arch.num_hidden_layers)
    pix = torch.randn(n, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(22)).to(dev, torch.bfloat16)
    eng = ClipVisionEngine(arch, sd, dev)
    if one_batch:
        eng.encode(pix)
        torch.cuda.synchronize()
        return
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    t_e = timed(lambda: eng.encode(pix), reps)
    t_r = timed(lambda: R.clip_vision_forward(sd_dev, arch, pix, dtype=torch.bfloat16, device=dev)["features"], reps)
    rec = dict(bench="clip_tower", arch="ViT-B/32", batch=n, reps=reps, engine_ms=round(t_e[0], 3), engine_ms_min=round(t_e[1], 3),
               engine_ms_max=round(t_e[2], 3), unfused_torch_ms=round(t_r[0], 3), unfused_torch_ms_min=round(t_r[1], 3),
               unfused_torch_ms_max=round(t_r[2], 3), engine_images_per_s=round(n / t_e[0] * 1e3, 1),
               unfused_torch_images_per_s=round(n / t_r[0] * 1e3, 1))
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "retrieval_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["topk", "tower"])
    ap.add_argument("--one-batch", action="store_true")
    a = ap.parse_args()
    if a.one_batch:
        return bench_tower(1, None, one_batch=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as out:
        if a.only != "tower":
            bench_topk(a.reps, out)
        if a.only != "topk":
            bench_tower(a.reps, out)


if __name__ == "__main__":
    main()
