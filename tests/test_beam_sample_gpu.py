"""licv_beam_sample_step (the SAMPLE path of csrc/beam.hip) step by step against the restatement: the Gumbel-top-k draw of
test_sampling_ref_cpu.py in front of the unchanged beam bookkeeping (oracle.generate_ref.beam_init + the bookkeeping half of
beam_step), with nb in {2, 3, 4, 8}, the KV row table included.  Integers exactly; scores to fp32 rounding (the kernel's
log-sum-exp is summed in another order than the restatement's)."""
import numpy as np
import pytest
import torch

import test_sampling_ref_cpu as R
from oracle import generate_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(B, nb, V, dtype, T, k, p, mp, seed, new=4, eos=2):
    from licv.generation import BeamSearchState, sample_params
    g = torch.Generator().manual_seed(seed)
    P = 3
    max_len = P + new
    ids = torch.randint(3, V, (B, P), generator=g)
    st = G.beam_init(ids, nb, max_len, eos, 0)
    st["V"] = V
    fill = eos
    table = torch.arange(B * nb, dtype=torch.int32)[:, None].repeat(1, max_len + 1).contiguous()
    dev = BeamSearchState(B, nb, P, max_len, fill, ids.to(DEV), eos, 1.0, False, 0, kv_rows=table.to(DEV),
                          sampling=sample_params(T, k, p, mp, seed))
    ref_rows = table.clone()
    first, steps = True, 0
    while True:
        rows = B if first else B * nb
        ld = (V + 7) // 8 * 8 + 8
        buf = (torch.randn(rows, ld, generator=g) * 2.0).to(dtype)
        logits = buf[:, :V].float()
        full = logits.repeat_interleave(nb, 0) if first else logits
        top_lp, top_ix, err = R.gumbel_select(full.view(B, nb, V).numpy(), st["run_scores"].numpy(), seed, st["cur"] - P, T,
                                              top_k=k, top_p=p, min_p=mp)
        if err:                                                       # too few candidates (a small kept set at step 0): both refuse
            with pytest.raises(ValueError):
                dev.step(buf.to(DEV)[:, :V], shared_rows=first)
            return dev
        cur = st["cur"]
        cont_ref, flat = R.beam_bookkeep(st, top_lp, top_ix, eos)
        new_rows = ref_rows[flat].clone()
        new_rows[:, cur] = torch.arange(B * nb, dtype=torch.int32)
        ref_rows = new_rows
        cont = dev.step(buf.to(DEV)[:, :V], shared_rows=first)
        first = False
        steps += 1
        d = dev.state[0]
        live = st["run_scores"] > -1e8
        assert torch.equal(d["run_scores"].cpu() > -1e8, live), f"step {steps}: live running beams"
        assert torch.equal(d["running"].cpu()[live], st["running"][live]), f"step {steps}: running token rows"
        assert torch.equal(d["is_fin"].cpu().bool(), st["is_fin"]), f"step {steps}: is_fin"
        fin = st["is_fin"]
        assert torch.equal(d["finished"].cpu()[fin], st["finished"][fin]), f"step {steps}: finished hypotheses"
        assert torch.equal(dev.kv_rows.cpu()[live.view(-1)], ref_rows[live.view(-1)]), f"step {steps}: KV row table"
        a_, b_ = d["run_scores"].cpu()[live], st["run_scores"][live]
        if bool(live.any()):
            assert (a_ - b_).abs().max() <= 2e-5 * (1 + b_.abs().max()), f"step {steps}: run_scores"
        assert cont == cont_ref, f"step {steps}: loop condition"
        if not cont:
            break
    return dev


@pytest.mark.parametrize("nb", [2, 3, 4, 8])
def test_beam_sample_step_equals_restatement(nb):
    for i, (dtype, V, T, k, p, mp) in enumerate(((torch.bfloat16, 32002, 1.0, 50, 1.0, 0.0), (torch.float32, 257, 0.7, 0, 0.9, 0.05),
                                                 (torch.bfloat16, 32003, 1.5, 50, 0.9, 0.0))):
        _run(3, nb, V, dtype, T, k, p, mp, seed=100 * nb + i)


def test_too_few_candidates_raises():
    """Step 0 with top_k = 1 and three beams: beam 0 keeps 2 tokens, beams 1.. carry -1e9 - fewer than 6 candidates of non-zero
    probability (torch.multinomial raises there)."""
    from licv.generation import BeamSearchState, sample_params
    B, nb, V, P = 2, 3, 257, 2
    ids = torch.randint(3, V, (B, P))
    dev = BeamSearchState(B, nb, P, P + 3, 2, ids.to(DEV), 2, 1.0, False, 0, sampling=sample_params(1.0, 1, 1.0, None, 5))
    with pytest.raises(ValueError):
        dev.step(torch.randn(B, V, device=DEV), shared_rows=True)
