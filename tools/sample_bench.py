"""Step times of the decode-step kernels of sampled generate at the idefics9b_generate_bs8 shape (8 questions x 3 beams x 32002
logits, bf16, padded row stride): licv_sample_step (8 rows, num_beams 1), licv_beam_sample_step (beam-search multinomial sampling)
beside licv_beam_step (beam search).  One JSON line per kernel; median of R repetitions of N back-to-back steps, events around
each batch.  Usage: python tools/sample_bench.py [--iters N] [--reps R] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "licv-vqa_amd"))
from licv.generation import BeamSearchState, SampleState, sample_params  # noqa: E402


def _time(fn, iters, reps):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    out.sort()
    return out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C
    from licv import _lib
    from licv.ops import _stream
    B, nb, V, P = 8, 3, 32002, 16
    ld = V + 14
    g = torch.Generator().manual_seed(0)
    lines = []
    for warp in ((1.0, 50, 1.0, None), (1.0, 0, 0.9, None), (0.7, 50, 0.9, 0.05)):
        p = sample_params(*warp, seed=1)
        x = (torch.randn(B, ld, generator=g) * 2).to(torch.bfloat16).cuda()[:, :V]
        seq = torch.zeros(B, P + 2, dtype=torch.long, device="cuda")
        unf = torch.ones(B, dtype=torch.uint8, device="cuda")
        nxt = torch.zeros(B, dtype=torch.long, device="cuda")
        flags = torch.zeros(1, dtype=torch.int32, device="cuda"); sync = torch.zeros(2, dtype=torch.int32, device="cuda")
        sa = _lib.SampleStepArgs()
        sa.logits, sa.logits_dtype, sa.ld, sa.B, sa.V = x.data_ptr(), 0, ld, B, V
        sa.ids, sa.ids_ld, sa.max_len, sa.cur, sa.P = seq.data_ptr(), P + 2, P + 2, P, P
        sa.unfinished, sa.next_tokens, sa.eos, sa.pad, sa.suppress_eos = unf.data_ptr(), nxt.data_ptr(), -1, 0, 0
        sa.flags, sa.sync = flags.data_ptr(), sync.data_ptr()
        L = _lib.lib()
        t = _time(lambda: L.licv_sample_step(C.byref(sa), C.byref(p), _stream(x)), a.iters, a.reps)
        lines.append(dict(kernel="licv_sample_step", B=B, V=V, dtype="bf16", temperature=warp[0], top_k=warp[1], top_p=warp[2],
                          min_p=warp[3], us=round(t, 2), target_us=30.0))
        xb = (torch.randn(B * nb, ld, generator=g) * 2).to(torch.bfloat16).cuda()[:, :V]
        ids = torch.zeros(B, P, dtype=torch.long, device="cuda")
        for kind in ("beam_step", "beam_sample_step"):
            bs = BeamSearchState(B, nb, P, P + 4, 2, ids, 2, 1.0, False, 0, sampling=p if kind == "beam_sample_step" else None)
            bs.step(xb)                                             # a state past step 0 (every beam live)

            def one():
                bs.cur = P + 1
                bs.step(xb)
            t = _time(one, a.iters, a.reps)
            lines.append(dict(kernel="licv_" + kind, B=B, nb=nb, V=V, dtype="bf16", temperature=warp[0], top_k=warp[1], top_p=warp[2],
                              min_p=warp[3], us_incl_host_readback=round(t, 2)))
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
