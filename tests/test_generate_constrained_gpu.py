"""Constrained hooked generate (repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens)
against the REFERENCE'S OWN bf16 decode: fixtures g20 / g21 (tools/make_golden_constrained.py) are the reference wrapper driving
transformers' generate with these keywords on tiny Idefics / Idefics2, hooks on, both padding sides, 8 new tokens, 3 beams
(length_penalty 0) and greedy.  Every row of every mode survived all jittered re-runs of the reference (every score moved by
-1 / 0 / +1 bf16 ulp), so the native engine must return every id of every row: no floor, no exemption.  Every mode changes at
least half of the rows (tests/test_logits_process_ref_cpu.py), so a decode that drops the keywords fails here.

Also: sampling without beams never emits a banned token and repeats when reseeded; beam-sampling with processors and bad
values raise."""
import pytest
import torch

from licv.config import IDEFICS2_TINY, IDEFICS_TINY
from licv.synthetic import synth_idefics2_weights, synth_idefics_weights

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
MODES = ("plain", "rep", "ngram", "bad", "suppress", "begin", "combo")


def _mode_kwargs(z, side):
    flat, offs = z[f"{side}_bad_words_flat"].tolist(), z[f"{side}_bad_words_offsets"].tolist()
    words = [flat[a:b] for a, b in zip(offs[:-1], offs[1:])]
    return dict(plain={}, rep=dict(repetition_penalty=1.5), ngram=dict(no_repeat_ngram_size=2), bad=dict(bad_words_ids=words),
                suppress=dict(suppress_tokens=z[f"{side}_suppress_tokens"].tolist()),
                begin=dict(begin_suppress_tokens=z[f"{side}_begin_suppress_tokens"].tolist()),
                combo=dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[z[f"{side}_combo_bad_word"].tolist()]))


def _check(w, icv, z, keys):
    bad = []
    for side in ("left", "right"):
        batch = {k: T(z[f"{side}_in_{k}"]).to(DEV) for k in keys}
        modes = _mode_kwargs(z, side)
        for tag, beams in (("beam", 3), ("greedy", 1)):
            for mode in MODES:
                got = w.generate(icv=icv, **batch, num_beams=beams, max_new_tokens=8, length_penalty=0.0, min_new_tokens=0, **modes[mode]).cpu()
                gold = T(z[f"{side}_{mode}_{tag}_ids"])
                assert bool((T(z[f"{side}_{mode}_{tag}_stability"]) >= 1.0).all())
                if got.shape != gold.shape:
                    bad.append((side, tag, mode, "shape", tuple(got.shape), tuple(gold.shape)))
                elif not torch.equal(got, gold):
                    bad.append((side, tag, mode, (got != gold).any(1).nonzero().flatten().tolist()))
    assert not bad, f"rows that differ from the reference's constrained bf16 decode: {bad}"


@pytest.fixture(scope="module")
def idefics(golden):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from lmm_icl_interface import IdeficsInterface
    z = golden("g20_generate_constrained")
    arch = IDEFICS_TINY.with_(additional_vocab_size=0)
    sd = synth_idefics_weights(arch, seed=int(z["weights_seed"]), dtype=torch.float32)
    sd["model.embed_tokens.weight"] *= float(z["embed_scale"])
    sd["lm_head.weight"] *= float(z["head_scale"])
    iface = IdeficsInterface(state_dict=sd, arch=arch, device=DEV)
    w = LearnableICVInterventionLMM(iface, True, -1, "model.model.layers.<LAYER_NUM>", arch.num_layers)
    return w, T(z["icv"]).to(DEV), z, arch


def test_idefics_constrained_generate_ids_match_the_reference(idefics):
    w, icv, z, _ = idefics
    _check(w, icv, z, ("input_ids", "attention_mask", "pixel_values", "image_attention_mask"))


def test_idefics2_constrained_generate_ids_match_the_reference(golden):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from lmm_icl_interface import Idefics2Interface
    z = golden("g21_generate_idefics2_constrained")
    arch = IDEFICS2_TINY
    sd = synth_idefics2_weights(arch, seed=int(z["weights_seed"]), dtype=torch.float32)
    sd["model.text_model.embed_tokens.weight"] *= float(z["embed_scale"])
    sd["lm_head.weight"] *= float(z["head_scale"])
    for l in range(arch.num_layers):
        sd[f"model.text_model.layers.{l}.mlp.down_proj.weight"] *= float(z["down_scale"])
    iface = Idefics2Interface(state_dict=sd, arch=arch, device=DEV)
    w = LearnableICVInterventionLMM(iface, True, -1, "model.model.text_model.layers.<LAYER_NUM>.mlp", arch.num_layers)
    _check(w, T(z["icv"]).to(DEV), z, ("input_ids", "attention_mask", "pixel_values", "pixel_attention_mask"))


def _batch(z, side="left"):
    return {k: T(z[f"{side}_in_{k}"]).to(DEV) for k in ("input_ids", "attention_mask", "pixel_values", "image_attention_mask")}


def test_sampling_without_beams_respects_the_bans_and_repeats_when_reseeded(idefics):
    w, icv, z, arch = idefics
    batch = _batch(z)
    P = batch["input_ids"].shape[1]
    banned = [t for t in range(3, arch.vocab_size, 2)]                  # half of the vocabulary
    begin = [t for t in range(4, arch.vocab_size, 4)]
    kw = dict(do_sample=True, num_beams=1, max_new_tokens=8, temperature=1.5, top_k=0, suppress_tokens=banned[:20],
              bad_words_ids=[[t] for t in banned[20:]], begin_suppress_tokens=begin, no_repeat_ngram_size=1)
    torch.manual_seed(7)
    a = w.generate(icv=icv, **batch, **kw).cpu()
    torch.manual_seed(7)
    b = w.generate(icv=icv, **batch, **kw).cpu()
    assert torch.equal(a, b)
    gen = a[:, P:]
    assert not bool(torch.isin(gen, torch.tensor(banned)).any())
    assert not bool(torch.isin(gen[:, 0], torch.tensor(begin)).any())
    for r in range(gen.shape[0]):                                       # n = 1: no token of the history again (until the row has ended)
        row = a[r].tolist()
        end = row.index(arch.eos_token_id, P) + 1 if arch.eos_token_id in row[P:] else len(row)
        assert all(row[i] not in row[:i] for i in range(P, end)), r
    torch.manual_seed(8)
    assert not torch.equal(a, w.generate(icv=icv, **batch, **kw).cpu())


def test_beam_sampling_with_processors_is_refused_and_bad_values_raise(idefics):
    w, icv, z, arch = idefics
    batch = _batch(z)
    with pytest.raises(NotImplementedError, match="num_beams"):
        w.generate(icv=icv, **batch, do_sample=True, num_beams=3, max_new_tokens=3, repetition_penalty=1.2)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=2), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=2.0), dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[arch.vocab_size]]),
               dict(bad_words_ids=[[-1]]), dict(suppress_tokens=[arch.vocab_size]), dict(begin_suppress_tokens=[-2])):
        with pytest.raises(ValueError):
            w.generate(icv=icv, **batch, max_new_tokens=3, **kw)
    # off values change nothing
    plain = w.generate(icv=icv, **batch, max_new_tokens=4)
    off = w.generate(icv=icv, **batch, max_new_tokens=4, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[], suppress_tokens=[])
    assert torch.equal(plain, off)
