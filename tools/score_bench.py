#!/usr/bin/env python3
"""Candidate ranking on a shared prompt (licv.generation.score_continuations) against the only way to get the same
numbers before it: engine.forward on the B*C concatenated [prompt | candidate] rows, all logits computed and all but a few rows
thrown away.  Synthetic weights at full width, B = 8 zero-shot prompts (Idefics-9B: 32 tokens, one image; Idefics2-8B: one 378x504
image, 64 <image> tokens + a 40-token question), C in {2, 16} candidates of 4 tokens, the hook on every layer.

Per (model, C): the median over `--reps` timed calls of the host clock around a call that ends in a device synchronise (the two
ways are timed alternately in one process, after `--warmup` calls of each), the row counts B*P + B*C*(T-1) against B*C*(P+T), and
the largest difference between the two ways' summed log-probabilities.  The vision side runs inside both.

    --kernel    also: one licv_append_attn call against the chain of T licv_decode_attn steps at the decode test's largest shapes -
                device-event medians and the share of output elements that are bit-equal

Prints one JSON line per measurement.  A missing GPU is an error, not a fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "licv-vqa_amd"))
sys.path.insert(0, str(ROOT))

B, T = 8, 4


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def model(preset, args):
    from licv import generation, ops
    from licv.config import idefics_arch
    from licv.synthetic import synth_icv
    dev = "cuda:0"
    arch = idefics_arch(preset)
    is2 = preset.startswith("idefics2")
    if is2:
        from licv.idefics2_engine import Idefics2Engine, Idefics2Weights
        from licv.synthetic import synth_idefics2_weights, synth_vqa_batch_idefics2
        eng = Idefics2Engine(Idefics2Weights(synth_idefics2_weights(arch, seed=426, dtype=torch.bfloat16, device=dev), arch, dev))
        P = arch.r_latents + 2 + 40
        batch = synth_vqa_batch_idefics2(arch, B, P, 1, 378, 504, seed=427, min_len=P - 8, dtype=torch.bfloat16, device=dev, ragged=False,
                                         padding_side="left")
        hi = arch.image_token_id - 1
    else:
        from licv.idefics_engine import IdeficsEngine, IdeficsWeights
        from licv.synthetic import synth_idefics_weights, synth_vqa_batch
        eng = IdeficsEngine(IdeficsWeights(synth_idefics_weights(arch, seed=426, dtype=torch.bfloat16, device=dev), arch, dev))
        P = 32
        batch = synth_vqa_batch(arch, B, P, 1, seed=427, min_len=P - 8, dtype=torch.bfloat16, device=dev, padding_side="left")
        hi = arch.vocab_size
    torch.cuda.empty_cache()
    icv, alpha = synth_icv(arch.num_layers, arch.hidden_size, seed=426, alpha=0.1, device=dev)
    hooks = dict(icv=alpha.unsqueeze(-1) * icv, hook_layers=list(range(arch.num_layers)))
    for C in args.candidates:
        g = torch.Generator().manual_seed(C)
        cand = torch.randint(3, hi, (B, C, T), generator=g).to(dev)
        lens = torch.full((B, C), T, device=dev)
        rep = lambda t: t.repeat_interleave(C, 0)
        ids = torch.cat([rep(batch["input_ids"]), cand.view(B * C, T)], 1)
        am = torch.cat([rep(batch["attention_mask"]), torch.ones((B * C, T), dtype=batch["attention_mask"].dtype, device=dev)], 1)
        rows = (torch.arange(B * C, device=dev)[:, None] * (P + T) + (P - 1) + torch.arange(T, device=dev)[None, :]).reshape(-1)

        if is2:
            pos = (am.long().cumsum(-1) - 1).masked_fill(am == 0, 0)
            pv, pam = rep(batch["pixel_values"]), rep(batch["pixel_attention_mask"])

            def shared():
                return generation.score_continuations_idefics2(eng, batch["input_ids"], batch["attention_mask"], batch["pixel_values"],
                                                               batch["pixel_attention_mask"], candidates=cand, candidate_lengths=lens, **hooks)

            def concat():
                return eng.forward(input_ids=ids, attention_mask=am, pixel_values=pv, pixel_attention_mask=pam, position_ids=pos, **hooks)
        else:
            iam = torch.cat([batch["image_attention_mask"], batch["image_attention_mask"][:, -1:].expand(-1, T, -1)], 1)
            pv, iam = rep(batch["pixel_values"]), rep(iam)

            def shared():
                return generation.score_continuations(eng, batch["input_ids"], batch["attention_mask"], batch["pixel_values"],
                                                      batch["image_attention_mask"], cand, lens, **hooks)

            def concat():
                return eng.forward(input_ids=ids, attention_mask=am, pixel_values=pv, image_attention_mask=iam, **hooks)

        def concat_scores():
            logits = concat()
            flat = logits.reshape(B * C * (P + T), -1) if logits.is_contiguous() else None
            if flat is None:                                                     # (B, S, V) view over rows with a padded stride
                flat = logits.as_strided((B * C * (P + T), logits.shape[-1]), (logits.stride(1), 1))
            return -ops.ce_rows(flat, rows, cand.reshape(-1), flat.shape[1]).view(B, C, T).sum(-1)

        for _ in range(args.warmup):
            shared()
            concat_scores()
        ts, tc = [], []
        for _ in range(args.reps):                                               # alternating: both see the same machine state
            ts += _timed(shared, 1)
            tc += _timed(concat_scores, 1)
        diff = float((shared().sum - concat_scores()).abs().max())
        ms_s, ms_c = statistics.median(ts), statistics.median(tc)
        print(json.dumps(dict(model=preset, B=B, C=C, T=T, P=P, rows_shared=B * P + B * C * (T - 1), rows_concat=B * C * (P + T),
                              shared_ms=round(ms_s, 3), shared_min_ms=round(min(ts), 3), shared_max_ms=round(max(ts), 3),
                              concat_ms=round(ms_c, 3), concat_min_ms=round(min(tc), 3), concat_max_ms=round(max(tc), 3),
                              concat_over_shared=round(ms_c / ms_s, 3), max_abs_score_diff=round(diff, 5), reps=args.reps)), flush=True)
    del eng
    torch.cuda.empty_cache()


def kernel(args):
    from licv import ops
    from oracle import idefics_ref as R
    dev = "cuda:0"
    for (M, nh, nkv, hd, past, Tn) in [(24, 32, 32, 128, 36, 4), (24, 32, 8, 128, 101, 16), (12, 32, 32, 128, 200, 32), (128, 32, 32, 128, 32, 3)]:
        g = torch.Generator().manual_seed(M + past)
        qd, kd = nh * hd, nkv * hd
        qkv = torch.randn(M * Tn, qd + 2 * kd, generator=g).to(torch.bfloat16).to(dev)
        cos, sin = (t.to(dev) for t in R.rotary_tables(hd, 512, 10000.0, torch.bfloat16))
        pos = (past + torch.arange(Tn)).repeat(M).to(dev)
        cache0 = torch.randn(M, past + Tn, 2 * kd, generator=g).to(torch.bfloat16).to(dev)
        rows = torch.arange(M, dtype=torch.int32).unsqueeze(1).repeat(1, past + Tn).to(dev)
        steps = [(qkv.view(M, Tn, -1)[:, t].contiguous(), pos.view(M, Tn)[:, t].contiguous()) for t in range(Tn)]
        c1, c2 = cache0.clone(), cache0.clone()

        def one():
            return ops.append_attn(qkv, cos, sin, pos, c1, past, Tn, nh, nkv, hd, hd ** -0.5, kv_rows=rows, append=True)

        def chain():
            return [ops.decode_attn(q, cos, sin, p, c2, past + t, nh, nkv, hd, hd ** -0.5, kv_rows=rows) for t, (q, p) in enumerate(steps)]

        res = {}
        for name, fn in (("append_attn_us", one), ("decode_chain_us", chain)):
            for _ in range(10):
                fn()
            ts = []
            for _ in range(100):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            res[name] = round(statistics.median(ts), 2)
        a = one().view(M, Tn, qd)
        b = torch.stack(chain(), 1)
        res["bit_equal_share"] = round(float((a == b).float().mean()), 5)
        res["max_abs_diff"] = float((a.float() - b.float()).abs().max())
        # history bytes: K and V rows of `past` positions per (row, kv head) - once, against once per step
        res["history_bytes_once"] = M * nkv * past * 2 * hd * 2
        res["history_bytes_chain"] = sum(M * nkv * (past + t) * 2 * hd * 2 for t in range(Tn))
        print(json.dumps(dict(kernel="licv_append_attn", M=M, nh=nh, nkv=nkv, hd=hd, past=past, T=Tn, **res)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="*", default=["idefics-9b", "idefics2-8b"])
    ap.add_argument("--candidates", type=int, nargs="*", default=[2, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench needs a GPU"
    with torch.no_grad():
        if args.kernel:
            kernel(args)
        for preset in args.models:
            model(preset, args)


if __name__ == "__main__":
    main()
