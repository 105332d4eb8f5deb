#!/usr/bin/env python3
"""Golden fixtures of CONSTRAINED hooked generate: g20 (tiny Idefics, additional_vocab_size=0) and g21 (tiny Idefics2).

Run in the build container only.  The set-ups are those of g15 / g16 in tools/make_golden.py: the reference's wrapper drives
the installed transformers `generate` on bf16 weights, hooks on, both padding sides.  Here max_new_tokens is 8, the decodes are
3 beams (length_penalty 0) and greedy, and each runs once per mode of transformers' built-in logits processors:

    plain      no processor (the unconstrained decode of the same prompts)
    rep        repetition_penalty=1.5
    ngram      no_repeat_ngram_size=2
    bad        bad_words_ids: every distinct first token of the pool's unconstrained decodes as a one-token word (EOS left
               out: NoBadWordsLogitsProcessor drops it) plus the most frequent generated bigram as a two-token word
    suppress   suppress_tokens: the most frequent third (at least 3) of those first tokens
    begin      begin_suppress_tokens: all of those first tokens
    combo      repetition_penalty=1.3, no_repeat_ngram_size=2 and the two-token bad word

Few prompts of these tiny models are decided by more than bf16 noise in all 14 decodes, so the candidate pool is wide.  A row
is a candidate when every mode's decode survives all jittered re-runs (every score moved by -1 / 0 / +1 bf16 ulp after the
built-in processors, see `_gen_with_margins`) and, in the `bad` and `begin` modes, differs from its unconstrained decode (a row
whose unconstrained first token is EOS does not).  Candidates that differ from their unconstrained decode in the most modes
are taken first; `_select_stable` then studies the kept batch again, in full.

The binding condition is asserted before a file is written: every mode changes at least half of the kept rows, `bad` and
`begin` all of them.  The weight seed of g21 was chosen among a dozen for a model whose decodes repeat themselves, so that the
penalty and the n-gram ban bind on stable rows (with seed 211 the n-gram ban bound on 1 - 4 of 8 kept rows, from a pool of 6144).
"""
from __future__ import annotations

import sys
from collections import Counter
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as M  # noqa: E402

NEW = 8
DECODES = (("beam", 3), ("greedy", 1))
MODES = ("plain", "rep", "ngram", "bad", "suppress", "begin", "combo")
MUST_BIND_ALL = ("bad", "begin")


def _rows_equal(a, b, fills):
    """Per row: the same decode (batches of different width: the common columns equal, the rest of the wider one only fill ids)."""
    n = min(a.shape[1], b.shape[1])
    rest = (a if a.shape[1] > n else b)[:, n:]
    return (a[:, :n] == b[:, :n]).all(1) & torch.isin(rest, torch.tensor(fills)).all(1)


def _word_lists(plain_ids, P, eos):
    """{mode: generate kwargs} from the pool's unconstrained decodes ({decode tag: ids})."""
    firsts, bigrams = Counter(), Counter()
    for ids in plain_ids.values():
        firsts.update(ids[:, P].tolist())
        gen = ids[:, P:]
        for r in range(gen.shape[0]):
            row = gen[r].tolist()
            bigrams.update((a, b) for a, b in zip(row[1:], row[2:]) if eos not in (a, b))
    first = sorted(firsts)
    one = [[t] for t in first if t != eos]
    two = list(bigrams.most_common(1)[0][0])
    some = sorted(t for t, _ in firsts.most_common(max(3, len(first) // 3)))
    return dict(plain={}, rep=dict(repetition_penalty=1.5), ngram=dict(no_repeat_ngram_size=2),
                bad=dict(bad_words_ids=one + [two]), suppress=dict(suppress_tokens=some), begin=dict(begin_suppress_tokens=first),
                combo=dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[two]))


def _build(out, w, icv, pool, n_pool, n_keep, P, eos, autocast):
    """One padding side: select the prompts, run every mode; returns {key suffix: array} for the fixture."""
    def gen(kw, beams, seed0, trials, gen_kw):
        gk = dict(max_new_tokens=NEW, **gen_kw)
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return M._gen_with_margins_seeded(w, icv, kw, beams, kw["input_ids"].shape[0], seed0, trials, gen_kw=gk)
        return M._gen_with_margins_seeded(w, icv, kw, beams, kw["input_ids"].shape[0], seed0, trials, gen_kw=gk)

    def batch_of(rows):
        b = pool if rows is None else {k: v[rows] for k, v in pool.items()}
        kw = dict(b)
        kw["pixel_values"] = b["pixel_values"].to(torch.bfloat16)
        return kw

    fills = [int(eos), int(w.lmm.tokenizer.pad_token_id)]
    w.toggle_intervention(True)
    plain_pool = {tag: gen(batch_of(None), beams, 1000, 0, {})[0] for tag, beams in DECODES}
    modes = _word_lists(plain_pool, P, eos)

    def pool_study(seed0, trials):
        """The study of the whole pool, staged: a row that fails a mode is not run in the later ones (a row's decode does not
        depend on its batch neighbours; `_select_stable` re-checks the kept rows together, in full), and 4 trials per mode come
        first, the rest only for the rows that survive them in every mode.  Returns the surviving rows, those that differ from
        their unconstrained decode in most modes first (stable rows bind less often than others: without the order the kept
        batch can fall under the binding condition)."""
        alive, binds = torch.arange(n_pool), {}
        for s0, n_trials in ((seed0, min(4, trials)), (seed0 + 4, trials - 4)):
            for tag, beams in DECODES:
                base = None
                for mode in MODES:
                    if n_trials <= 0 or len(alive) == 0:
                        break
                    ids, st = gen(batch_of(alive.tolist()), beams, s0, n_trials, modes[mode])
                    ok = st >= 1.0
                    if mode == "plain":
                        base = ids
                    else:
                        binds[f"{mode}_{tag}"] = ~_rows_equal(ids, base, fills)
                        if mode in MUST_BIND_ALL:
                            ok &= binds[f"{mode}_{tag}"]
                    alive, base, binds = alive[ok], base[ok], {k: v[ok] for k, v in binds.items()}
                    print(f"    pool, {n_trials} trials, {mode}/{tag}: {len(alive)} rows left", flush=True)
        count = torch.stack(list(binds.values())).sum(0)
        order = torch.argsort(count, descending=True, stable=True)
        print(f"    {len(alive)} stable rows, modes that bind per row (sorted): {count[order].tolist()}", flush=True)
        return alive[order].tolist()

    def study(rows, seed0, trials):
        if rows is None:                                      # the candidates below are the pool study's survivors
            return {"all": (None, torch.ones(len(cands)))}
        rows = [cands[i] for i in rows]
        kw = batch_of(rows)
        res = {}
        print(f"    kept rows {rows}: {trials} trials in every mode", flush=True)
        for tag, beams in DECODES:
            for mode in MODES:
                ids, st = gen(kw, beams, seed0, trials, modes[mode])
                if mode in MUST_BIND_ALL:                     # a row these modes leave unchanged is not a candidate
                    st = torch.where(_rows_equal(ids, res[f"plain_{tag}"][0], fills), torch.zeros_like(st), st)
                res[f"{mode}_{tag}"] = (ids, st)
        return res

    cands = pool_study(1000, 24)
    keep, res = M._select_stable(study, len(cands), n_keep, 24)
    keep = [cands[i] for i in keep]
    for k, v in pool.items():
        out[f"in_{k}"] = M.np_(v[keep])
    for tag, _ in DECODES:
        base = res[f"plain_{tag}"][0]
        for mode in MODES:
            ids, st = res[f"{mode}_{tag}"]
            assert bool((st >= 1.0).all())
            out[f"{mode}_{tag}_ids"], out[f"{mode}_{tag}_stability"] = ids.numpy(), st.numpy()
            if mode != "plain":
                changed = int((~_rows_equal(ids, base, fills)).sum())
                print(f"    {mode}/{tag}: {changed}/{n_keep} rows differ from the unconstrained decode", flush=True)
                assert changed * 2 >= n_keep, f"{mode}/{tag} binds on {changed} of {n_keep} rows only: widen the pool"
                assert mode not in MUST_BIND_ALL or changed == n_keep
    bad = modes["bad"]["bad_words_ids"]
    out["bad_words_flat"] = np.array([t for wd in bad for t in wd], dtype=np.int64)
    out["bad_words_offsets"] = np.cumsum([0] + [len(wd) for wd in bad]).astype(np.int64)
    out["suppress_tokens"] = np.array(modes["suppress"]["suppress_tokens"], dtype=np.int64)
    out["begin_suppress_tokens"] = np.array(modes["begin"]["begin_suppress_tokens"], dtype=np.int64)
    out["combo_bad_word"] = np.array(modes["combo"]["bad_words_ids"][0], dtype=np.int64)


def _g20_side(side):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    arch = M.IDEFICS_TINY.with_(additional_vocab_size=0)
    seed, POOL, B = 201, 3072, 8
    out = {}
    sd32 = M.synth_idefics_weights(arch, seed=seed, dtype=torch.float32)
    out["weights_checksum"] = np.array(M.weights_checksum(sd32))
    out["embed_scale"], out["head_scale"], out["weights_seed"] = np.array(25.0), np.array(10.0), np.array(seed)
    sd32["model.embed_tokens.weight"] *= 25.0
    sd32["lm_head.weight"] *= 10.0
    icv = torch.randn(1, arch.num_layers, arch.hidden_size, generator=torch.Generator().manual_seed(seed + 1)) * 0.2
    out["icv"] = M.np_(icv)
    model = M.hf_model(arch, sd32, torch.bfloat16)
    model.generation_config.pad_token_id = arch.pad_token_id
    iface = M.Interface(model, arch.pad_token_id)
    print(f"g20 {side}", flush=True)
    pool = M.synth_vqa_batch(arch, POOL, 12, 1, seed=seed + (0 if side == "left" else 7), min_len=9 if side == "left" else 12,
                             dtype=torch.float32, padding_side=side)
    w = LearnableICVInterventionLMM(iface, True, -1, "model.model.layers.<LAYER_NUM>", arch.num_layers)
    part = {}
    _build(part, w, icv, pool, POOL, B, 12, arch.eos_token_id, autocast=False)
    out.update({f"{side}_{k}": v for k, v in part.items()})
    return out


def _g21_side(side):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    arch = M.IDEFICS2_TINY
    seed, POOL, B = 215, 4096, 16
    out = {}
    sd32 = M.synth_idefics2_weights(arch, seed=seed, dtype=torch.float32)
    out["weights_checksum"] = np.array(M.weights_checksum(sd32))
    out["embed_scale"], out["head_scale"], out["down_scale"] = np.array(25.0), np.array(10.0), np.array(40.0)
    out["weights_seed"] = np.array(seed)
    sd32["model.text_model.embed_tokens.weight"] *= 25.0
    sd32["lm_head.weight"] *= 10.0
    for l in range(arch.num_layers):
        sd32[f"model.text_model.layers.{l}.mlp.down_proj.weight"] *= 40.0
    icv = torch.randn(1, arch.num_layers, arch.hidden_size, generator=torch.Generator().manual_seed(seed + 1)) * 0.2
    out["icv"] = M.np_(icv)
    model = M.hf_idefics2(arch, sd32, torch.bfloat16)
    model.generation_config.pad_token_id = arch.pad_token_id
    model.generation_config.eos_token_id = arch.eos_token_id
    iface = M.Interface(model, arch.pad_token_id)
    print(f"g21 {side}", flush=True)
    pool = M.synth_vqa_batch_idefics2(arch, POOL, 20, 2, 56, 42, seed=seed + (0 if side == "left" else 7),
                                      min_len=15 if side == "left" else 20, dtype=torch.float32, padding_side=side)
    w = LearnableICVInterventionLMM(iface, True, -1, "model.model.text_model.layers.<LAYER_NUM>.mlp", arch.num_layers)
    part = {}
    _build(part, w, icv, pool, POOL, B, 20, arch.eos_token_id, autocast=True)
    out.update({f"{side}_{k}": v for k, v in part.items()})
    return out


def _setup():
    M.OUT.mkdir(parents=True, exist_ok=True)
    M._install_shims()
    sys.path.insert(0, str(M.REF))
    import icv_src.icv_model.icv_intervention as _ri
    assert _ri.__file__.startswith(str(M.REF)), _ri.__file__
    torch.set_num_threads(4)


def main():
    """The two padding sides of a fixture are studied in two processes (each builds the same seeded model)."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    table = dict(g20=(_g20_side, "g20_generate_constrained"), g21=(_g21_side, "g21_generate_idefics2_constrained"))
    for name in sys.argv[1:] or list(table):
        print("==", name, flush=True)
        fn, file = table[name]
        with ProcessPoolExecutor(2, mp_context=mp.get_context("spawn"), initializer=_setup) as ex:
            out = {}
            for part in ex.map(fn, ("left", "right")):
                out.update(part)
        np.savez_compressed(M.OUT / f"{file}.npz", **out)


if __name__ == "__main__":
    main()
