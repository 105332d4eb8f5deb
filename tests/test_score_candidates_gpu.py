"""score_continuations / score_continuations_idefics2 (licv/generation.py): closed-set scoring of candidate answers on a shared prompt.
Gold is the CPU oracle's plain forward on the B*C concatenated [prompt | candidate] rows (for Idefics every candidate token takes
the image-mask row of the prompt's last token), in bf16 and in fp32; the per-token log-probabilities are held to
tests/test_engine_gpu.py's bars (i) and (ii), bar (ii) calibrated by the oracle's own bf16-to-fp32 spread on those log-probabilities.
Ranking: the arg-max candidate equals the fp32 oracle's wherever the fp32 top-2 margin exceeds that spread.  B = 3 left-padded
prompts of unequal length, C = 4 candidates of 1 .. 5 tokens, hooks off and on all layers.

The seeds below were picked on the CPU with the oracle alone (`python tests/test_score_candidates_gpu.py` prints, per configuration,
how many questions the margin condition keeps): every configuration keeps at least 2 of its 3 questions."""
import functools

import pytest
import torch

from licv.config import IDEFICS2_MID, IDEFICS2_TINY, IDEFICS_MID, IDEFICS_TINY
from licv.synthetic import (synth_idefics2_weights, synth_idefics_weights, synth_vqa_batch, synth_vqa_batch_idefics2)

DEV = "cuda"
B, C, T = 3, 4, 5
ARCHS = {"idefics_tiny": IDEFICS_TINY, "idefics_mid": IDEFICS_MID, "idefics2_tiny": IDEFICS2_TINY, "idefics2_mid": IDEFICS2_MID}
SEEDS = {"idefics_tiny": 11, "idefics_mid": 11, "idefics2_tiny": 11, "idefics2_mid": 11}
CASES = [(name, hooked) for name in ARCHS for hooked in (False, True)]
CASE_IDS = [f"{n}-{'hooked' if h else 'plain'}" for n, h in CASES]


def _is2(name):
    return name.startswith("idefics2")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Weights (fp32 state dict), the prompt batch, the candidates and the vector: CPU tensors, never modified."""
    arch, seed = ARCHS[name], SEEDS[name]
    g = torch.Generator().manual_seed(seed)
    if _is2(name):
        sd = synth_idefics2_weights(arch, seed=seed, dtype=torch.float32)
        P = arch.r_latents + 12
        batch = synth_vqa_batch_idefics2(arch, B, P, 1, 2 * arch.v_patch, 2 * arch.v_patch, seed=seed + 1, min_len=P - 5, dtype=torch.float32,
                                         ragged=False, padding_side="left")
        hi = arch.image_token_id - 1
    else:
        sd = synth_idefics_weights(arch, seed=seed, dtype=torch.float32)
        P = 16
        batch = synth_vqa_batch(arch, B, P, 1, seed=seed + 1, min_len=P - 5, dtype=torch.float32, padding_side="left")
        hi = arch.vocab_size - 2
    assert int(batch["attention_mask"].sum(1).min()) < P and bool((batch["attention_mask"][:, -1] == 1).all())
    lens = torch.randint(1, T + 1, (B, C), generator=g)
    lens[0, 0], lens[0, 1] = 1, T                                         # both ends of the range are present
    cand = torch.randint(3, hi, (B, C, T), generator=g)
    cand = torch.where(torch.arange(T)[None, None, :] < lens[:, :, None], cand, torch.zeros((), dtype=torch.long))
    icv = torch.randn(1, arch.num_layers, arch.hidden_size, generator=g) * 0.05
    return sd, batch, cand, lens, icv


@functools.lru_cache(maxsize=None)
def _gold(name, hooked):
    """{dtype name: (B, C, T) fp32 per-token log-probabilities of the oracle on the concatenated rows, zero at padding}."""
    arch = ARCHS[name]
    sd32, batch, cand, lens, icv = _inputs(name)
    layers = list(range(arch.num_layers))
    hooks = dict(icv=icv, hook_layers=layers) if hooked else {}
    P = batch["input_ids"].shape[1]
    valid = torch.arange(T)[None, None, :] < lens[:, :, None]
    rep = lambda t: t.repeat_interleave(C, 0)
    ids = torch.cat([rep(batch["input_ids"]), cand.view(B * C, T)], 1)
    am = torch.cat([rep(batch["attention_mask"]), valid.view(B * C, T).long()], 1)
    out = {}
    for dname, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        sd = {k: v.to(dt) for k, v in sd32.items()}
        with torch.no_grad():
            if _is2(name):
                from oracle import idefics2_ref as R2
                feats = R2.image_features(batch["pixel_values"].to(dt), batch["pixel_attention_mask"], sd, arch)
                feats = rep(feats.view(B, -1, feats.shape[-1])).reshape(-1, feats.shape[-1])
                pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 0)           # HF's generate-time position ids
                # (bf16 with the fp32 vector: the reference runs under autocast, as tests/test_idefics2_gpu.py's oracle calls do)
                with torch.autocast("cpu", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                    logits = R2.forward(sd, arch, ids, am, image_hidden_states=feats, position_ids=pos, **hooks)
            else:
                from oracle import idefics_ref as R
                states = R.image_states_from_pixels(batch["pixel_values"].to(dt), sd, arch)
                iam = batch["image_attention_mask"]
                iam = torch.cat([iam, iam[:, -1:].expand(-1, T, -1)], 1)     # every candidate token: the mask row of the prompt's last token
                logits = R.forward(sd, arch, ids, am, image_attention_mask=rep(iam), image_states=rep(states), **hooks)
        lp = torch.log_softmax(logits[:, P - 1:P - 1 + T].float(), -1).gather(-1, cand.view(B * C, T, 1)).view(B, C, T)
        out[dname] = torch.where(valid, lp, torch.zeros(()))
    return out


def _spreads(gold):
    tok = float((gold["bf16"] - gold["f32"]).abs().max())
    tot = float((gold["bf16"].sum(-1) - gold["f32"].sum(-1)).abs().max())
    return tok, tot


def _kept(gold):
    """Questions whose fp32 top-2 margin (of the summed scores) exceeds the oracle's bf16-to-fp32 spread of those scores."""
    top2 = gold["f32"].sum(-1).topk(2, -1).values
    return (top2[:, 0] - top2[:, 1]) > _spreads(gold)[1]


@functools.lru_cache(maxsize=None)
def _engine(name, use_runner=True):
    sd32 = _inputs(name)[0]
    if _is2(name):
        from licv.idefics2_engine import Idefics2Engine, Idefics2Weights
        return Idefics2Engine(Idefics2Weights(sd32, ARCHS[name], DEV))
    from licv.idefics_engine import IdeficsEngine, IdeficsWeights
    return IdeficsEngine(IdeficsWeights(sd32, ARCHS[name], DEV), use_runner=use_runner)


def _score(name, hooked, engine=None, cand=None, lens=None, batch=None, **kw):
    from licv import generation
    arch = ARCHS[name]
    _, batch0, cand0, lens0, icv = _inputs(name)
    batch = batch0 if batch is None else batch
    cand, lens = (cand0 if cand is None else cand), (lens0 if lens is None else lens)
    hooks = dict(icv=icv.to(DEV), hook_layers=list(range(arch.num_layers))) if hooked else {}
    engine = _engine(name) if engine is None else engine
    b = {k: v.to(DEV) for k, v in batch.items()}
    if _is2(name):
        return generation.score_continuations_idefics2(engine, b["input_ids"], b["attention_mask"], b["pixel_values"].to(torch.bfloat16),
                                                       b["pixel_attention_mask"], candidates=cand.to(DEV), candidate_lengths=lens.to(DEV), **hooks, **kw)
    return generation.score_continuations(engine, b["input_ids"], b["attention_mask"], b["pixel_values"].to(torch.bfloat16),
                                          b["image_attention_mask"], cand.to(DEV), lens.to(DEV), **hooks, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,hooked", CASES, ids=CASE_IDS)
def test_token_logprobs_and_ranking_against_the_oracle(name, hooked):
    gold = _gold(name, hooked)
    _, _, cand, lens, _ = _inputs(name)
    res = _score(name, hooked)
    got = res.token_logprobs.cpu()
    assert got.shape == (B, C, T) and got.dtype == torch.float32
    valid = torch.arange(T)[None, None, :] < lens[:, :, None]
    assert bool((got[~valid] == 0).all()), "zero at padding"
    assert torch.allclose(res.sum.cpu(), got.sum(-1)) and torch.allclose(res.mean.cpu(), got.sum(-1) / lens.float())
    scale = float(gold["f32"].abs().max())
    e_gold = float((got - gold["bf16"]).abs().max())
    e_true = float((got - gold["f32"]).abs().max())
    spread, _ = _spreads(gold)
    print(f"{name} hooked={hooked}: |hip-bf16| {e_gold:.3e} |hip-f32| {e_true:.3e} spread {spread:.3e} scale {scale:.3e}")
    assert e_gold <= 1.5e-2 * scale, f"|hip-bf16 gold| {e_gold:.3e} vs scale {scale:.3e}"
    assert e_true <= 1.5 * spread + 1e-3 * scale, f"|hip-f32 gold| {e_true:.3e} vs reference spread {spread:.3e}"
    kept = _kept(gold)
    assert int(kept.sum()) * 2 >= B, "the margin condition may leave out at most half of the questions"
    best, want = res.sum.cpu().argmax(-1), gold["f32"].sum(-1).argmax(-1)
    assert torch.equal(best[kept], want[kept])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["idefics_tiny", "idefics2_tiny"])
def test_one_token_candidates_need_no_continuation_pass(name, monkeypatch):
    from licv import generation, ops
    calls = []
    real = ops.append_attn
    monkeypatch.setattr(ops, "append_attn", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _, batch, cand, lens, _ = _inputs(name)
    engine = _engine(name, use_runner=False) if not _is2(name) else _engine(name)      # the Python loop: every launch goes through licv.ops
    res = _score(name, True, engine=engine, cand=cand[:, :, :2], lens=torch.ones_like(lens))
    assert not calls, "no licv_append_attn launch when every candidate is one token long"
    assert res.token_logprobs.shape == (B, C, 1)
    # ... and the result is licv_ce_rows on the prefill's last-row logits, bit for bit
    arch = ARCHS[name]
    b = {k: v.to(DEV) for k, v in batch.items()}
    hooks = dict(icv=_inputs(name)[4].to(DEV), hook_layers=list(range(arch.num_layers)))
    P = b["input_ids"].shape[1]
    last = generation._last_rows(B, P, DEV)
    if _is2(name):
        pos = (b["attention_mask"].long().cumsum(-1) - 1).masked_fill(b["attention_mask"] == 0, 0)
        logits = engine.forward(input_ids=b["input_ids"], attention_mask=b["attention_mask"], pixel_values=b["pixel_values"].to(torch.bfloat16),
                                pixel_attention_mask=b["pixel_attention_mask"], position_ids=pos, logits_rows=last, **hooks)
    else:
        logits = engine.forward(input_ids=b["input_ids"], attention_mask=b["attention_mask"], pixel_values=b["pixel_values"].to(torch.bfloat16),
                                image_attention_mask=b["image_attention_mask"], logits_rows=last, **hooks)
    ce = ops.ce_rows(logits, torch.arange(B, device=DEV).repeat_interleave(C), cand[:, :, 0].reshape(-1).to(DEV), logits.shape[1])
    assert torch.equal(res.token_logprobs.view(-1), -ce) and torch.equal(res.sum.view(-1), -ce)
    # with longer candidates the counter does move: one launch per layer and chunk
    _score(name, True, engine=engine)
    assert len(calls) == arch.num_layers
    calls.clear()
    _score(name, True, engine=engine, max_rows=2 * B)                     # C = 4 candidates in chunks of 2
    assert len(calls) == 2 * arch.num_layers


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["idefics_tiny", "idefics_mid"])
def test_runner_and_python_loop_agree_bit_for_bit(name):
    a = _score(name, True, engine=_engine(name, use_runner=True))
    b = _score(name, True, engine=_engine(name, use_runner=False))
    assert torch.equal(a.token_logprobs, b.token_logprobs)
    a = _score(name, False, engine=_engine(name, use_runner=True), max_rows=2 * B)
    b = _score(name, False, engine=_engine(name, use_runner=False), max_rows=2 * B)
    assert torch.equal(a.token_logprobs, b.token_logprobs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["idefics_tiny", "idefics2_tiny"])
def test_scoring_twice_and_generate_afterwards(name):
    from licv import generation
    arch = ARCHS[name]
    _, batch, _, _, icv = _inputs(name)
    b = {k: v.to(DEV) for k, v in batch.items()}
    hooks = dict(icv=icv.to(DEV), hook_layers=list(range(arch.num_layers)))

    def gen(engine):
        if _is2(name):
            return generation.generate_idefics2(engine, b["input_ids"], b["attention_mask"], b["pixel_values"].to(torch.bfloat16),
                                                b["pixel_attention_mask"], max_new_tokens=4, num_beams=3, **hooks).cpu()
        return generation.generate(engine, b["input_ids"], b["attention_mask"], b["pixel_values"].to(torch.bfloat16), b["image_attention_mask"],
                                   max_new_tokens=4, num_beams=3, **hooks).cpu()
    fresh = gen(_engine.__wrapped__(name))
    engine = _engine.__wrapped__(name)
    one, two = _score(name, True, engine=engine), _score(name, True, engine=engine)
    assert torch.equal(one.token_logprobs, two.token_logprobs) and torch.equal(one.sum, two.sum) and torch.equal(one.mean, two.mean)
    assert torch.equal(gen(engine), fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["idefics_tiny", "idefics2_tiny"])
def test_wrapper_and_interface_pass_through_like_generate(name):
    """LearnableICVInterventionLMM.score_candidates(icv=...) -> the interface's score_candidates: the hook plan and the toggle apply."""
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from lmm_icl_interface import Idefics2Interface, IdeficsInterface
    arch = ARCHS[name]
    sd32, batch, cand, lens, icv = _inputs(name)
    fmt = "model.model.text_model.layers.<LAYER_NUM>.mlp" if _is2(name) else "model.model.layers.<LAYER_NUM>"
    iface = (Idefics2Interface if _is2(name) else IdeficsInterface)(state_dict=sd32, arch=arch, device=DEV)
    w = LearnableICVInterventionLMM(iface, True, -1, fmt, arch.num_layers)
    b = {k: v.to(DEV) for k, v in batch.items()}
    b["pixel_values"] = b["pixel_values"].to(torch.bfloat16)
    on = w.score_candidates(icv=icv.to(DEV), **b, candidates=cand, candidate_lengths=lens)
    assert torch.equal(on.token_logprobs, _score(name, True, engine=iface.engine).token_logprobs)
    w.toggle_intervention(False)
    off = w.score_candidates(icv=icv.to(DEV), **b, candidates=cand, candidate_lengths=lens)
    assert torch.equal(off.token_logprobs, _score(name, False, engine=iface.engine).token_logprobs)
    assert not torch.equal(on.token_logprobs, off.token_logprobs)


@pytest.mark.gpu
def test_errors():
    from licv._lib import APPEND_MAX_T
    name = "idefics_tiny"
    _, batch, cand, lens, _ = _inputs(name)
    right = dict(batch)
    right["attention_mask"] = batch["attention_mask"].flip(1)              # right padded: some row's last column is masked
    with pytest.raises(ValueError, match="left padded"):
        _score(name, False, batch=right)
    long = torch.ones((B, C, APPEND_MAX_T + 2), dtype=torch.long)
    with pytest.raises(ValueError, match=f"LICV_APPEND_MAX_T = {APPEND_MAX_T}"):
        _score(name, False, cand=long, lens=torch.full((B, C), APPEND_MAX_T + 2))
    with pytest.raises(ValueError):
        _score(name, False, lens=torch.zeros_like(lens))


if __name__ == "__main__":                                                # seed picking, on the CPU with the oracle alone
    for n, h in CASES:
        g_ = _gold(n, h)
        print(n, "hooked" if h else "plain", "kept", int(_kept(g_).sum()), "of", B, "spreads", _spreads(g_))
