"""licv_beam_step fed FINAL log-probabilities (logits_dtype = LICV_F32_LOGPROBS, `BeamSearchState.step(..., logprobs_in=True)`): what
licv_logits_process leaves with normalize = 1, rows that hold -inf where a processor banned a token.  Step by step against the
oracle's beam step (oracle/generate_ref.beam_step) given the SAME log-probabilities - its log_softmax is switched off for the
call, the rows are final - with the equalities of tests/test_beam_step_gpu.py: integers and booleans exactly, scores to fp32
rounding (here lp = x + running score on both sides)."""
import ctypes as C

import pytest
import torch

from oracle import generate_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _oracle_step(monkeypatch, st, lp, eos, lpen, early, sup):
    # oracle/ may not change, so its log_softmax is made the identity for this one call: the rows are final log-probabilities.
    # beam_step calls torch.log_softmax exactly once (on the logits it is given, oracle/generate_ref.py); the counter below holds
    # that, so that a second use added there one day cannot be switched off here unnoticed.
    calls = []

    def identity(x, dim=-1):
        calls.append(1)
        return x
    with monkeypatch.context() as m:
        m.setattr(torch, "log_softmax", identity)
        out = G.beam_step(st, lp, eos, lpen, early, suppress_eos=sup)
    assert len(calls) == 1
    return out


def _run(monkeypatch, B, nb, V, P, new, eos, lpen, early, min_new, seed):
    from licv.generation import BeamSearchState
    g = torch.Generator().manual_seed(seed)
    max_len, pad = P + new, 0
    ids = torch.randint(3, V, (B, P), generator=g)
    st = G.beam_init(ids, nb, max_len, eos, pad)
    dev = BeamSearchState(B, nb, P, max_len, eos, ids.to(DEV), eos, lpen, early, min_new)
    first, steps = True, 0
    while True:
        rows = B if first else B * nb
        ld = V + 5
        buf = torch.randn(rows, ld, generator=g)
        n_top = 6 * nb                                                  # a decided top without ties, as tests/test_beam_step_gpu.py builds it
        for r in range(rows):
            toks = torch.randperm(V, generator=g)[:n_top]
            buf[r, toks] = 6.0 + 0.75 * torch.arange(n_top, dtype=torch.float32)[torch.randperm(n_top, generator=g)] + 0.25 * torch.rand(n_top, generator=g)
            if float(torch.rand((), generator=g)) < 0.3:
                buf[r, eos] = 6.0 + 0.75 * (n_top - 1) + 0.375
        lp = torch.log_softmax(buf[:, :V], -1)
        banned = torch.rand(rows, V, generator=g) < 0.2                 # what the processors did: -inf, the row's best token among them
        banned[torch.arange(rows), lp.argmax(-1)] = True
        buf[:, :V] = lp.masked_fill(banned, float("-inf"))
        lp = buf[:, :V]
        sup = min_new > 0 and st["cur"] - P < min_new
        cont_ref, flat_ref = _oracle_step(monkeypatch, st, lp.repeat_interleave(nb, 0) if first else lp.clone(), eos, lpen, early, sup)
        cont = dev.step(buf.to(DEV)[:, :V], shared_rows=first, logprobs_in=True)
        first = False
        steps += 1
        d = dev.state[0]
        live = st["run_scores"] > -1e8
        assert torch.equal(d["run_scores"].cpu() > -1e8, live), f"step {steps}: live running beams"
        assert torch.equal(d["running"].cpu()[live], st["running"][live]), f"step {steps}: running token rows"
        assert torch.equal(d["is_fin"].cpu().bool(), st["is_fin"]), f"step {steps}: is_fin"
        assert torch.equal(d["improve"].cpu().bool().view(-1, 1), st["improve"]), f"step {steps}: improve"
        fin = st["is_fin"]
        assert torch.equal(d["gen_len"].cpu()[fin], st["gen_len"][fin]) and torch.equal(d["finished"].cpu()[fin], st["finished"][fin]), \
            f"step {steps}: finished hypotheses"
        for k, m in (("run_scores", live), ("fin_scores", fin)):
            a_, b_ = d[k].cpu(), st[k]
            if bool(m.any()):
                assert (a_[m] - b_[m]).abs().max() <= 2e-5 * (1 + b_[m].abs().max()), f"step {steps}: {k}"
            assert bool((a_[~m] < -1e8).all()) and bool((b_[~m] < -1e8).all()), f"step {steps}: dead {k}"
        assert cont == cont_ref, f"step {steps}: loop condition"
        assert int(dev.sync.abs().sum()) == 0
        if not cont:
            break
        lf = live.reshape(-1)
        assert torch.equal(dev.beam_src_flat.cpu()[lf], flat_ref[lf]), f"step {steps}: KV-cache reorder indices"
        assert torch.equal(dev.next_tokens.cpu()[lf], st["running"][:, :, st["cur"] - 1].reshape(-1)[lf]), f"step {steps}: next tokens"
    assert torch.equal(dev.result().cpu(), st["finished"][:, 0, : P + int(st["gen_len"][:, 0].max())])
    return steps


@pytest.mark.parametrize("nb", [2, 3])
def test_beam_step_on_final_logprobs_matches_the_oracle_step_by_step(monkeypatch, nb):
    total = 0
    for seed, (B, V, P, new, eos, lpen, early, min_new) in enumerate([
            (4, 32002, 7, 5, 2, 0.0, False, 0), (3, 1000, 4, 8, 2, 0.7, True, 0), (5, 500, 5, 7, 2, 1.3, False, 3)]):
        total += _run(monkeypatch, B, nb, V, P, new, eos, lpen, early, min_new, 300 * nb + seed)
    assert total >= 9


def test_beam_sample_step_rejects_final_logprobs():
    from licv import _lib
    from licv.generation import BeamSearchState, sample_params
    B, nb, V, P = 2, 2, 64, 3
    ids = torch.randint(3, V, (B, P)).to(DEV)
    s = BeamSearchState(B, nb, P, P + 4, 2, ids, 2, 1.0, False, 0, sampling=sample_params(seed=1))
    with pytest.raises(_lib.LicvError, match="logprobs_in"):
        s.step(torch.zeros((B, V), device=DEV), shared_rows=True, logprobs_in=True)
