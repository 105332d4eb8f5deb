#!/usr/bin/env python3
"""One decode step's attention block over short and long histories: licv_decode_attn, the single launch with one
wave per (row, kv head), against licv_decode_attn_split, split-key attention + merge, with the plan's choice of splits and with
n_splits in {1, 2, 4, 8, 16, 32}.  M in {24, 8} rows (8 questions x 3 beams; 8 greedy rows), 32 query heads on 32 or 8 kv heads,
head_dim 128, Sk in {37, 101, 800, 2900, 10000} keys, and the split entry alone at Sk = 12000, which the single launch refuses.
bf16 QKV rows, an identity row table, every key visible.

Per measurement: the median over 100 calls (after 10 warm-up calls) of the time between two device events around ONE call through
the C ABI with a workspace allocated beforehand (for the short histories this includes what the host needs to issue one or two
launches), and the share of output elements that are bit-equal to licv_decode_attn's.

Prints one JSON line per (shape, entry); profiles/decode_attn_bench.txt is this output.  A missing GPU is an error, not a fallback."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "licv-vqa_amd"))
sys.path.insert(0, str(ROOT))

SPLITS = (1, 2, 4, 8, 16, 32)


def _median_us(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(ts), 2)


def shape(M, nh, nkv, hd, Sk, args):
    from licv import _lib, ops
    from oracle import idefics_ref as R
    dev = "cuda:0"
    past = Sk - 1
    g = torch.Generator(device=dev).manual_seed(M * 100003 + nkv * 1009 + Sk)
    qd, kd = nh * hd, nkv * hd
    qkv = torch.randn(M, qd + 2 * kd, generator=g, device=dev).to(torch.bfloat16)
    cos, sin = (t.to(dev) for t in R.rotary_tables(hd, 512, 10000.0, torch.bfloat16))
    pos = torch.randint(0, 512, (M,), generator=g, device=dev)
    cache = torch.randn(M, Sk, 2 * kd, generator=g, device=dev, dtype=torch.bfloat16)
    rows = torch.arange(M, dtype=torch.int32, device=dev).unsqueeze(1).repeat(1, Sk).contiguous()
    out = torch.empty((M, qd), dtype=torch.bfloat16, device=dev)
    a = _lib.DecodeAttnArgs()
    a.qkv_bf16, a.ldq = qkv.data_ptr(), qkv.stride(0)
    a.cos, a.sin, a.position_ids, a.n_pos = cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), cos.shape[0]
    a.cache, a.max_len, a.past = cache.data_ptr(), cache.shape[1], past
    a.kv_rows, a.ld_kv_rows = rows.data_ptr(), rows.shape[1]
    a.out, a.M, a.n_heads, a.n_kv_heads, a.head_dim, a.scale = out.data_ptr(), M, nh, nkv, hd, hd ** -0.5
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan_n, _ = ops.decode_attn_split_plan(M, nh, nkv, hd, Sk)
    ws = torch.empty((M * nh * _lib.DECODE_MAX_SPLITS * (hd + 2),), dtype=torch.float32, device=dev)
    base = dict(M=M, nh=nh, nkv=nkv, hd=hd, Sk=Sk)
    ref = None
    if Sk <= 10240:
        single = lambda: _lib.check(lib.licv_decode_attn(C.byref(a), stream))
        us = _median_us(single, args.warmup, args.reps)
        ref = out.clone()
        print(json.dumps(dict(**base, entry="licv_decode_attn", us=us)), flush=True)
    sweeps = (Sk + 63) // 64
    for n in [0] + sorted({min(n, sweeps) for n in SPLITS}):           # a wish above the sweep count is clamped to it: measured once
        split = lambda: _lib.check(lib.licv_decode_attn_split(C.byref(a), n, C.c_void_p(ws.data_ptr()), ws.numel() * 4, stream))
        us = _median_us(split, args.warmup, args.reps)
        rec = dict(**base, entry="licv_decode_attn_split", n_splits=("plan:%d" % plan_n) if n == 0 else n, us=us)
        if ref is not None:
            d = (out.float() - ref.float()).abs()
            rec.update(bit_equal_share=round(float((out == ref).float().mean()), 5), max_abs_diff=float(d.max()))
        print(json.dumps(rec), flush=True)
    del cache
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="*", default=[24, 8])
    ap.add_argument("--keys", type=int, nargs="*", default=[37, 101, 800, 2900, 10000, 12000])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_attn_bench needs a GPU"
    with torch.no_grad():
        for M in args.rows:
            for nkv in (32, 8):
                for Sk in args.keys:
                    shape(M, 32, nkv, 128, Sk, args)


if __name__ == "__main__":
    main()
