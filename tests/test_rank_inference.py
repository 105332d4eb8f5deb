"""`rank_answers` / `rank_inference` of the inference mirror with a stub model (its `score_candidates` returns a fixed table) and a stub
tokenizer: candidates tokenised as given and right padded, the vector scaled by alpha, the bs-wide last chunk, "sum" against
"mean", the record's form, the caller's samples left alone.  No GPU."""
import types

import pytest
import torch

import inference as I


class FakeTokenizer:
    """One token per character: id = 10 + (ord(c) - ord('a')); a space is token 3.  add_special_tokens must be False."""
    pad_token_id, bos_token_id, eos_token_id, padding_side = 0, 1, 2, "left"

    def __init__(self):
        self.calls = []

    def __call__(self, text, add_special_tokens=True):
        assert add_special_tokens is False, "candidates are tokenised without special tokens"
        self.calls.append(text)
        return {"input_ids": [3 if c == " " else 10 + ord(c) - ord("a") for c in text]}


class StubModel:
    """score_candidates returns rows of a fixed (C, T) table of per-token log-probabilities, masked by the lengths it is given."""

    def __init__(self, table):
        self.table, self.calls = table, []
        self.lmm = types.SimpleNamespace(device=torch.device("cpu"))

    def score_candidates(self, icv=None, candidates=None, candidate_lengths=None, **kw):
        self.calls.append(dict(icv=icv, candidates=candidates.clone(), candidate_lengths=candidate_lengths.clone(), **kw))
        B, C, T = candidates.shape
        lp = self.table[None, :C, :T].expand(B, C, T).clone()
        lp = lp * (torch.arange(T)[None, None, :] < candidate_lengths[:, :, None])
        s = lp.sum(-1)
        return types.SimpleNamespace(token_logprobs=lp, sum=s, mean=s / candidate_lengths.float())


# "no" is short and unlikely per token; "maybe" is long and likely per token: the sum prefers "no", the mean prefers "maybe"
TABLE = torch.tensor([[-1.5, -1.5, 0.0, 0.0, 0.0], [-0.8, -0.8, -0.8, -0.8, -0.8], [-2.0, -2.0, -2.0, 0.0, 0.0]])
CANDS = ["no", "maybe", " ab"]


def _inputs(n):
    return dict(input_ids=torch.full((n, 3), 4), attention_mask=torch.ones(n, 3, dtype=torch.long))


def test_rank_answers_tokenises_pads_scales_and_ranks():
    tok = FakeTokenizer()
    proc = types.SimpleNamespace(tokenizer=tok)
    model = StubModel(TABLE)
    vec = torch.arange(6, dtype=torch.float32).reshape(1, 2, 3)
    alpha = torch.tensor([[0.5, 2.0]])
    best, scores = I.rank_answers(_inputs(2), model, proc, [CANDS, CANDS], in_context_vector=vec, alpha=alpha)
    call = model.calls[0]
    assert torch.equal(call["icv"], alpha.unsqueeze(-1) * vec)
    assert call["candidates"].shape == (2, 3, 5) and call["candidates"].dtype == torch.int64
    assert call["candidates"][0].tolist() == [[10 + 13, 10 + 14, 0, 0, 0], [22, 10, 34, 11, 14], [3, 10, 11, 0, 0]]       # as given (leading space kept), right padded
    assert call["candidate_lengths"].tolist() == [[2, 5, 3]] * 2
    assert torch.equal(call["input_ids"], _inputs(2)["input_ids"])
    assert tok.calls == CANDS * 2
    assert best == [0, 0]                                               # sum: -3.0 against -4.0 and -6.0
    assert scores[0] == pytest.approx([-3.0, -4.0, -6.0])
    best, scores = I.rank_answers(_inputs(2), model, proc, CANDS, normalize="mean")      # one list for every row; no vector
    assert model.calls[1]["icv"] is None
    assert best == [1, 1]                                               # mean: -0.8 against -1.5 and -2.0
    assert scores[1] == pytest.approx([-1.5, -0.8, -2.0])
    with pytest.raises(ValueError):
        I.rank_answers(_inputs(2), model, proc, CANDS, normalize="median")
    with pytest.raises(ValueError):
        I.rank_answers(_inputs(2), model, proc, [CANDS, CANDS[:2]])


def test_rank_inference_batches_keeps_last_chunk_wide_and_builds_records():
    tok = FakeTokenizer()
    seen = []

    def prepare_input(prompts):
        seen.append(prompts)
        return _inputs(len(prompts))

    proc = types.SimpleNamespace(tokenizer=tok, prepare_input=prepare_input)
    pm = types.SimpleNamespace(gen_query_text_without_label=lambda s: f"Question:{s['question']} Short answer:")
    ds = [dict(image=f"img{i}", question=f"q{i}", question_id=i, choices=list(CANDS)) for i in range(5)]
    model = StubModel(TABLE)
    vec, alpha = torch.ones(1, 2, 3), torch.tensor([[2.0, 3.0]])
    res = I.rank_inference(ds, model, pm, proc, bs=2, candidates=CANDS, instruction="Answer briefly.", in_context_vector=vec, alpha=alpha)
    assert list(res) == [0, 1, 2, 3, 4]
    assert res[3] == {"prediction": "no", "scores": pytest.approx([-3.0, -4.0, -6.0]), "question": "q3", "question_id": 3, "choices": CANDS}
    assert [len(p) for p in seen] == [2, 2, 2]                                           # last chunk still bs prompts wide
    assert seen[2][1] == ["Answer briefly."]                                             # ... the spare one instruction-only
    assert seen[0][0] == ["Answer briefly.", "img0", "Question:q0 Short answer:"]
    assert all(c["candidates"].shape[0] == 2 for c in model.calls)
    assert torch.equal(model.calls[0]["icv"], alpha.unsqueeze(-1) * vec)
    assert "image" in ds[0] and ds[0]["choices"] == CANDS                                # caller's samples are not mutated
    # candidates named by a per-sample field, ranked by the mean
    res = I.rank_inference(ds, model, pm, proc, bs=2, candidates="choices", normalize="mean")
    assert res[4]["prediction"] == "maybe" and res[4]["scores"] == pytest.approx([-1.5, -0.8, -2.0])
    assert "image" not in res[4] and model.calls[-1]["icv"] is None
