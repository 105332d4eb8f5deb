#!/usr/bin/env python3
"""Time of the logits-processor pre-pass of one decode step (licv_logits_process) at the beam-search shape of
the headline workload: R = 24 rows (8 questions x 3 beams), V = 32002, a history of 820 tokens, all five processors on.

    --gpu   median of the device-event time of one call on cuda:0 (warmed, the stream fenced before and after every sample; a
            batch of back-to-back calls is timed as well: the per-call time without the event overhead)
    --cpu   the same five transformers processor classes on the same rows on the CPU (what the pre-pass replaces)

Prints one JSON line per mode.  A missing GPU with --gpu is an error, not a fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "licv-vqa_amd"))

R, V, CUR, P, N = 24, 32002, 820, 815, 3


def rows(seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(R, V + 30, generator=g) * 4.0).to(torch.bfloat16)
    ids = torch.randint(0, V, (R, CUR + 8), generator=g)
    ids[:, 1::3] = torch.randint(0, 200, (R, len(range(1, CUR + 8, 3))), generator=g)       # repeated tokens and n-grams
    words = [[int(t)] for t in torch.randint(3, V, (30,), generator=g)] + [[32000, 32001], [5, 6, 7]]
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=N, bad_words_ids=words,
              suppress_tokens=[int(t) for t in torch.randint(3, V, (16,), generator=g)],
              begin_suppress_tokens=[int(t) for t in torch.randint(3, V, (16,), generator=g)])
    return logits, ids, kw


def gpu():
    assert torch.cuda.is_available(), "--gpu needs a GPU"
    from licv.ops import LogitsConstraints, logits_process
    logits, ids, kw = rows()
    lg, idd = logits.cuda()[:, :V], ids.cuda()
    cons = LogitsConstraints("cuda", eos=2, **kw)
    out = torch.empty((R, V), dtype=torch.float32, device="cuda")
    res = {}
    for name, cur, norm in (("beam_step", CUR, True), ("greedy_step", CUR, False), ("first_step", P, True)):
        for _ in range(20):
            logits_process(lg, idd, cur, P, cons, normalize=norm, out=out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            logits_process(lg, idd, cur, P, cons, normalize=norm, out=out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            logits_process(lg, idd, cur, P, cons, normalize=norm, out=out)
        torch.cuda.synchronize()
        batch = (time.perf_counter() - t0) / 500 * 1e6
        res[name] = dict(event_median_us=round(statistics.median(ts), 2), event_p10_us=round(sorted(ts)[20], 2),
                         event_p90_us=round(sorted(ts)[180], 2), back_to_back_us=round(batch, 2))
    print(json.dumps(dict(mode="gpu", R=R, V=V, history=CUR, **res)))


def cpu():
    from transformers.generation import logits_process as L
    logits, ids, kw = rows()
    scores = torch.log_softmax(logits[:, :V].float(), -1)
    procs = [L.RepetitionPenaltyLogitsProcessor(penalty=kw["repetition_penalty"]), L.NoRepeatNGramLogitsProcessor(N),
             L.NoBadWordsLogitsProcessor(kw["bad_words_ids"], 2), L.SuppressTokensLogitsProcessor(kw["suppress_tokens"]),
             L.SuppressTokensAtBeginLogitsProcessor(kw["begin_suppress_tokens"], P)]
    h = ids[:, :CUR]
    ts = []
    for i in range(25):
        t0 = time.perf_counter()
        s = scores
        for p in procs:
            s = p(h, s)
        if i >= 5:
            ts.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(dict(mode="cpu", R=R, V=V, history=CUR, threads=torch.get_num_threads(), median_us=round(statistics.median(ts), 1))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    if a.cpu:
        cpu()
    if a.gpu:
        gpu()
