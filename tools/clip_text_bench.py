"""CLIP text tower measurements: texts/s of the packed tower and the time of its ragged causal attention kernel
(licv_attn_varlen_causal) at the openai/clip-vit-base-patch32 text width, 512 texts, twice: every text 77 tokens long (what padding
to the model's maximum costs), and lengths drawn uniformly from 6..20 (what VQA questions look like).  One JSON line per run, appended
to profiles/clip_text_bench.jsonl.

  python tools/clip_text_bench.py [--out profiles/clip_text_bench.jsonl] [--reps 20] [--texts 512]

Device-event timing, warm-up, median of --reps (min and max beside it).  The tower's time includes the host side of a batch (packing,
the copies of ids / positions / cu_seqlens to the device): that is what encode_text pays per batch."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "licv-vqa_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def batch(arch, lens):
    rng = np.random.default_rng(7)
    S = int(max(lens))
    ids = np.full((len(lens), S), arch.vocab_size - 1, dtype=np.int64)
    mask = np.zeros((len(lens), S), dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(3, arch.vocab_size - 2, n)
        ids[i, 0], ids[i, n - 1] = arch.vocab_size - 2, arch.vocab_size - 1
        mask[i, :n] = 1
    return torch.from_numpy(ids), torch.from_numpy(mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip_text_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--texts", type=int, default=512)
    a = ap.parse_args()
    from licv import ops
    from licv.clip_engine import ClipTextEngine, pack_text_batch
    from licv.config import CLIP_TEXT_B32 as arch
    from licv.synthetic import synth_clip_text_weights, trained_like_
    dev = torch.device("cuda:0")
    sd = trained_like_(synth_clip_text_weights(arch, seed=24, dtype=torch.bfloat16), arch.num_hidden_layers)
    eng = ClipTextEngine(arch, sd, dev)
    runs = [("all_77", np.full(a.texts, 77)), ("uniform_6_20", np.random.default_rng(8).integers(6, 21, a.texts))]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as out:
        for name, lens in runs:
            ids, mask = batch(arch, lens)
            pk = pack_text_batch(ids, mask, arch)
            total, E = int(pk.cu_seqlens[-1]), arch.hidden_size
            t_tower = timed(lambda: eng.encode(ids, mask), a.reps)
            qkv = torch.randn(total, 3 * E, generator=torch.Generator().manual_seed(9)).to(dev, torch.bfloat16)
            cu_dev = pk.cu_seqlens.to(dev)
            o = torch.empty((total, E), dtype=torch.bfloat16, device=dev)
            t_attn = timed(lambda: ops.attn_varlen_causal(qkv, pk.cu_seqlens, cu_dev, arch.num_attention_heads, arch.head_dim,
                                                          arch.head_dim ** -0.5, out=o), a.reps)
            rec = dict(bench="clip_text", arch="B/32 text", run=name, texts=int(a.texts), tokens=total, padded_tokens=int(a.texts * ids.shape[1]),
                       tokens_at_77=int(a.texts * 77), reps=a.reps,
                       tower_ms=round(t_tower[0], 3), tower_ms_min=round(t_tower[1], 3), tower_ms_max=round(t_tower[2], 3),
                       texts_per_s=round(a.texts / t_tower[0] * 1e3, 1),
                       attn_varlen_us=round(t_attn[0] * 1e3, 1), attn_varlen_us_min=round(t_attn[1] * 1e3, 1),
                       attn_varlen_us_max=round(t_attn[2] * 1e3, 1), attn_share_of_tower=round(arch.num_hidden_layers * t_attn[0] / t_tower[0], 4))
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
