"""Sampled hooked generate at toy widths (IDEFICS_TINY, IDEFICS2_TINY): every step's native logits are recorded and fed to the CPU
restatement (test_sampling_ref_cpu.py), whose ids must equal the native ids for num_beams 1 and 3 with hooks on and off;
do_sample with top_k = 1 is greedy; torch.manual_seed reproduces a run; `inference.generate_answers` with sampling kwargs returns
strings through LearnableICVInterventionLMM; an unbuilt warper kwarg raises."""
import types

import numpy as np
import pytest
import torch

import test_sampling_ref_cpu as R
from licv.config import IDEFICS2_TINY, IDEFICS_TINY
from licv.synthetic import synth_idefics2_weights, synth_idefics_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMT = "model.model.layers.<LAYER_NUM>"


def _iface():
    from lmm_icl_interface import IdeficsInterface
    arch = IDEFICS_TINY.with_(additional_vocab_size=0)
    return IdeficsInterface(state_dict=synth_idefics_weights(arch, seed=21, dtype=torch.float32), arch=arch, device=DEV), arch


def _batch(golden):
    z = golden("g5_generate")
    return {k: torch.from_numpy(z[f"left_in_{k}"]).to(DEV) for k in ("input_ids", "attention_mask", "pixel_values", "image_attention_mask")}


class _Recorder:
    """Wraps SampleState.step / BeamSearchState.step: keeps every step's logits (as fp32 on the host) and the state before it."""

    def __init__(self, monkeypatch):
        from licv import generation
        self.steps = []
        rec = self
        s0, b0 = generation.SampleState.step, generation.BeamSearchState.step

        def sstep(st, logits):
            rec.steps.append(("s", logits.float().cpu(), st.unfinished.cpu().numpy().astype(bool), st.cur, st.sampling.seed))
            return s0(st, logits)

        def bstep(st, logits, shared_rows=False):
            rec.steps.append(("b", logits.float().cpu(), shared_rows, st.cur, st.sampling.seed if st.sampling else None))
            return b0(st, logits, shared_rows=shared_rows)

        monkeypatch.setattr(generation.SampleState, "step", sstep)
        monkeypatch.setattr(generation.BeamSearchState, "step", bstep)


def _replay(rec, ids, P, nb, eos, pad, warp, max_new=5):
    """The restatement's ids from the recorded logits."""
    from oracle import generate_ref as G
    B = ids.shape[0]
    T = warp.get("temperature") or 1.0
    w = dict(top_k=50 if warp.get("top_k") is None else warp["top_k"], top_p=warp.get("top_p") or 1.0, min_p=warp.get("min_p") or 0.0)
    if nb == 1:
        seq = [ids.cpu().numpy()]
        unf = np.ones(B, dtype=bool)
        for _, logits, _, cur, seed in rec.steps:
            tok, unf = R.sample_step(logits.numpy(), seed, cur - P, unf, eos, pad, False, T, **w)
            seq.append(tok[:, None])
        return torch.from_numpy(np.concatenate(seq, 1))
    st = G.beam_init(ids.cpu(), nb, P + max_new, eos, pad)
    st["V"] = rec.steps[0][1].shape[1]
    for _, logits, shared, cur, seed in rec.steps:
        full = logits.repeat_interleave(nb, 0) if shared else logits
        top_lp, top_ix, err = R.gumbel_select(full.view(B, nb, -1).numpy(), st["run_scores"].numpy(), seed, cur - P, T, **w)
        assert not err
        R.beam_bookkeep(st, top_lp, top_ix, eos)
    return st["finished"][:, 0, : P + int(st["gen_len"][:, 0].max())]


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("hooks", [True, False])
def test_sampled_generate_equals_restatement(golden, monkeypatch, nb, hooks):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    iface, arch = _iface()
    batch = _batch(golden)
    w = LearnableICVInterventionLMM(iface, True, -1, FMT, arch.num_layers)
    w.toggle_intervention(hooks)
    icv = torch.randn(1, arch.num_layers, arch.hidden_size, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.1
    rec = _Recorder(monkeypatch)
    warp = dict(temperature=0.8, top_p=0.9)
    torch.manual_seed(4)
    out = w.generate(icv=icv, **batch, num_beams=nb, max_new_tokens=5, do_sample=True, **warp).cpu()
    P = batch["input_ids"].shape[1]
    assert len(rec.steps) >= 1 and all(s[0] == ("s" if nb == 1 else "b") for s in rec.steps)
    want = _replay(rec, batch["input_ids"], P, nb, arch.eos_token_id, arch.pad_token_id, warp)
    assert torch.equal(out, want[:, : out.shape[1]]) and out.shape == want.shape


def test_top_k_one_is_greedy(golden):
    iface, arch = _iface()
    batch = _batch(golden)
    greedy = iface.generate(**batch, num_beams=1, max_new_tokens=5).cpu()
    sampled = iface.generate(**batch, num_beams=1, max_new_tokens=5, do_sample=True, top_k=1).cpu()
    assert torch.equal(greedy, sampled)


def test_manual_seed_reproduces_and_idefics2_samples():
    from lmm_icl_interface import Idefics2Interface
    arch = IDEFICS2_TINY
    iface = Idefics2Interface(state_dict=synth_idefics2_weights(arch, seed=5, dtype=torch.float32), arch=arch, device=DEV)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, arch.vocab_size, (4, 7), generator=g).to(DEV)
    am = torch.ones_like(ids)
    runs = []
    for s in (9, 9, 10):
        torch.manual_seed(s)
        runs.append(iface.generate(input_ids=ids, attention_mask=am, num_beams=1, max_new_tokens=6, do_sample=True, top_k=0,
                                   temperature=1.5).cpu())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    torch.manual_seed(9)
    b = iface.generate(input_ids=ids, attention_mask=am, num_beams=3, max_new_tokens=4, do_sample=True, top_p=0.9).cpu()
    assert b.shape[0] == 4 and b.shape[1] >= 8


def test_generate_answers_with_sampling_kwargs(golden):
    """ref:inference.py generate_answers with generate_kwargs that add do_sample to the shipped config (num_beams 3)."""
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from inference import generate_answers
    iface, arch = _iface()
    batch = _batch(golden)
    w = LearnableICVInterventionLMM(iface, True, -1, FMT, arch.num_layers)

    class Tok:
        def batch_decode(self, rows, skip_special_tokens=False):
            return [" ".join(str(t) for t in r) for r in rows]

    proc = types.SimpleNamespace(tokenizer=Tok())
    icv = torch.randn(1, arch.num_layers, arch.hidden_size, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.1
    torch.manual_seed(1)
    texts = generate_answers(batch, w, proc, {"do_sample": True, "num_beams": 3, "top_p": 0.9, "max_new_tokens": 5},
                             in_context_vector=icv, alpha=torch.ones(1, arch.num_layers, device=DEV))
    assert len(texts) == batch["input_ids"].shape[0] and all(isinstance(t, str) for t in texts)


@pytest.mark.parametrize("kw", ["typical_p", "top_h", "epsilon_cutoff", "eta_cutoff"])
def test_unbuilt_warper_raises(golden, kw):
    iface, _ = _iface()
    with pytest.raises(NotImplementedError, match=kw):
        iface.generate(**_batch(golden), num_beams=1, max_new_tokens=2, do_sample=True, **{kw: 0.5})
