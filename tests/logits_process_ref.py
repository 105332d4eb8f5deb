"""Plain-torch restatement of the five logits processors licv_logits_process builds (csrc/logits_process.hip) and of its two modes:
the test oracle where transformers is not a dependency.  Semantics and order are transformers 5.x `_get_logits_processor`
(generation/utils.py) with generation/logits_process.py's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor;
tests/test_logits_process_ref_cpu.py holds this file equal to those classes."""
import torch

NEG_INF = float("-inf")


def process(scores, ids, P, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None,
            begin_suppress_tokens=None, eos=None):
    """scores: (R, V) fp32 (logits, or log-probabilities in beam search); ids: (R, cur) int64 history, the first P columns the prompt.
    Returns new (R, V) fp32 scores.  Every entry is its input, one fp32 product or quotient of it, or -inf."""
    assert scores.dtype == torch.float32 and ids.dim() == 2 and ids.shape[0] == scores.shape[0]
    R, V = scores.shape
    cur = ids.shape[1]
    out = scores.clone()
    if repetition_penalty != 1.0:
        theta = torch.tensor(repetition_penalty, dtype=torch.float32)
        seen = torch.zeros((R, V), dtype=torch.bool)
        seen.scatter_(1, ids, True)                                   # a token seen twice is penalised once
        out = torch.where(seen, torch.where(scores < 0, scores * theta, scores / theta), scores)
    ban = torch.zeros((R, V), dtype=torch.bool)
    n = no_repeat_ngram_size
    if n > 0 and cur >= n:
        for r in range(R):
            h = ids[r].tolist()
            suffix = h[cur - n + 1:]
            for i in range(cur - n + 1):
                if h[i:i + n - 1] == suffix:
                    ban[r, h[i + n - 1]] = True
    for word in bad_words_ids or []:
        word = list(word)
        if eos is not None and word == [eos]:
            continue
        L = len(word)
        if L == 1:
            ban[:, word[0]] = True
        elif L <= cur:                                                # a word longer than the history is ignored
            hit = (ids[:, cur - (L - 1):] == torch.tensor(word[:-1])).all(1)
            ban[hit, word[-1]] = True
    for t in suppress_tokens or []:
        ban[:, t] = True
    if cur == P:
        for t in begin_suppress_tokens or []:
            ban[:, t] = True
    return out.masked_fill(ban, NEG_INF)


def log_softmax_rows(logits):
    """The normalize = 1 input: fp32 log-softmax of the fp32 value of the logits (what `_beam_search` hands to the processors)."""
    return torch.log_softmax(logits.float(), dim=-1)
