"""tests/logits_process_ref.py (the oracle of the GPU tests of licv_logits_process) against the installed transformers processor
classes, exactly (every processor is one IEEE operation per entry or a -inf write), and the constrained-generate fixtures g20 /
g21 (tools/make_golden_constrained.py): every row stable under the bf16-ulp jitter, every mode binding."""
import numpy as np
import pytest
import torch

from logits_process_ref import process

EOS = 2


def _rows(seed, R, V, cur, P):
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(R, V, generator=g) * 3.0                     # both signs
    scores[:, ::7] = scores[:, ::7].abs()
    ids = torch.randint(0, V, (R, cur), generator=g)
    if cur >= 4:
        ids[:, 1] = ids[:, 0]                                         # duplicate history tokens
        ids[0, -1] = ids[0, 0]                                        # the last token seen before: n-gram windows match
        ids[1, -2:] = ids[1, :2]
    return scores, ids


def _hf(scores, ids, P, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None,
        begin_suppress_tokens=None):
    """transformers' own classes in _get_logits_processor's order."""
    L = pytest.importorskip("transformers.generation.logits_process")
    s = scores.clone()
    if repetition_penalty != 1.0:
        s = L.RepetitionPenaltyLogitsProcessor(penalty=repetition_penalty)(ids, s)
    if no_repeat_ngram_size > 0:
        s = L.NoRepeatNGramLogitsProcessor(no_repeat_ngram_size)(ids, s)
    if bad_words_ids:
        s = L.NoBadWordsLogitsProcessor(bad_words_ids, EOS)(ids, s)
    if suppress_tokens:
        s = L.SuppressTokensLogitsProcessor(suppress_tokens)(ids, s)
    if begin_suppress_tokens:
        s = L.SuppressTokensAtBeginLogitsProcessor(begin_suppress_tokens, P)(ids, s)
    return s


def _same(a, b):
    return torch.equal(a, b) and torch.equal(torch.isinf(a), torch.isinf(b))


@pytest.mark.parametrize("cur,P", [(1, 1), (2, 1), (3, 3), (9, 9), (9, 4), (40, 33)])
def test_restatement_equals_the_transformers_processors(cur, P):
    pytest.importorskip("transformers")
    R, V = 5, 50
    scores, ids = _rows(10 * cur + P, R, V, cur, P)
    h = ids[2].tolist()
    words = [[7], [EOS],                                              # a word equal to [eos] is dropped
             h[-2:] + [11] if cur >= 2 else [5, 11],                  # matches row 2
             [(h[-1] + 1) % V, 12],                                   # nearly matches (wrong prefix)
             [(h[0] + 1) % V] + h[1:] + [13],                         # nearly matches, as long as the history + 1: ignored
             h + [14],                                                # prefix = the whole history: longer than hf accepts
             list(range(cur + 3))]                                    # longer than the history
    cases = [dict(repetition_penalty=1.5), dict(repetition_penalty=0.7),
             dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=3),
             dict(no_repeat_ngram_size=cur + 1), dict(no_repeat_ngram_size=cur + 2),       # cur + 1 == n and cur + 1 < n
             dict(bad_words_ids=words), dict(suppress_tokens=[0, 3, V - 1]), dict(begin_suppress_tokens=[1, 4, V - 2]),
             dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=words, suppress_tokens=[3], begin_suppress_tokens=[4])]
    for kw in cases:
        got, ref = process(scores, ids, P, eos=EOS, **kw), _hf(scores, ids, P, **kw)
        assert _same(got, ref), (kw, cur, P)
    # on log-probabilities (beam search): negative everywhere, -inf present
    lp = torch.log_softmax(scores, -1)
    lp[:, 5] = float("-inf")
    kw = cases[-1]
    assert _same(process(lp, ids, P, eos=EOS, **kw), _hf(lp, ids, P, **kw))


def test_penalty_is_applied_once_and_bans_bind():
    scores = torch.tensor([[2.0, -2.0, 1.0, -1.0, 0.5, 0.25]])
    ids = torch.tensor([[0, 0, 1, 1, 4]])
    out = process(scores, ids, 2, repetition_penalty=2.0)
    assert out.tolist() == [[1.0, -4.0, 1.0, -1.0, 0.25, 0.25]]
    out = process(scores, ids, 5, no_repeat_ngram_size=2, bad_words_ids=[[1, 4, 3]], begin_suppress_tokens=[5], suppress_tokens=[2])
    assert torch.isinf(out).tolist() == [[False, False, True, True, False, True]]      # nothing follows a 4 yet; [1, 4] -> 3; 2; 5 at cur == P
    assert torch.isinf(process(scores, ids[:, :4], 2, no_repeat_ngram_size=2)).tolist() == [[False, True, False, False, False, False]]


MODES = ("rep", "ngram", "bad", "suppress", "begin", "combo")


def _equal_rows(a, b, fills):
    n = min(a.shape[1], b.shape[1])
    rest = (a if a.shape[1] > n else b)[:, n:]
    return (a[:, :n] == b[:, :n]).all(1) & np.isin(rest, fills).all(1)


@pytest.mark.parametrize("fixture,eos,pad", [("g20_generate_constrained", 2, 0), ("g21_generate_idefics2_constrained", 2, 0)])
def test_constrained_fixtures_are_stable_and_binding(golden, fixture, eos, pad):
    z = golden(fixture)
    for side in ("left", "right"):
        for tag in ("beam", "greedy"):
            base = z[f"{side}_plain_{tag}_ids"]
            assert (z[f"{side}_plain_{tag}_stability"] >= 1.0).all()
            for mode in MODES:
                ids = z[f"{side}_{mode}_{tag}_ids"]
                assert (z[f"{side}_{mode}_{tag}_stability"] >= 1.0).all(), (side, mode, tag)
                changed = int((~_equal_rows(ids, base, [eos, pad])).sum())
                assert changed * 2 >= len(ids), f"{side}/{mode}/{tag}: only {changed} of {len(ids)} rows differ from the unconstrained decode"
                if mode in ("bad", "begin"):
                    assert changed == len(ids), (side, mode, tag)
        offs = z[f"{side}_bad_words_offsets"]
        assert offs[0] == 0 and (np.diff(offs) > 0).all() and offs[-1] == len(z[f"{side}_bad_words_flat"])
