"""Hooked greedy / beam-search decoding on the native engine (ref:inference.py:300-321 `generate_answers`;
ref:config/inference.yaml:26-30: max_new_tokens 5, num_beams 3, length_penalty 0.0, min_new_tokens 0).

The search bookkeeping restates transformers' ``GenerationMixin._sample`` / ``_beam_search`` (5.x vectorised
form: top-2K continuations, running vs finished beam sets, the ``early_stopping=False`` heuristic) so that
token ids are bit-identical for identical logits.  The model side is the native engine: one prefill on B rows
(the KV cache is then replicated per beam instead of prefilling B*beams identical rows), then single-token
steps on (B*beams, 1) with the ICV hook firing at every step, as in the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .idefics_engine import IdeficsEngine, KVCache


def _last_rows(B: int, S: int, dev) -> torch.Tensor:
    return torch.arange(B, device=dev) * S + (S - 1)


class _shared_prompt:
    """For one continuation step: the cache's row table maps row r to the prompt row r // cc, and nothing is appended.  The cache (rows,
    len, cross-attention K|V) is as before afterwards."""

    def __init__(self, cache: KVCache, cc: int):
        self.cache, self.cc = cache, cc

    def __enter__(self):
        c = self.cache
        self.saved = (c.rows, c.append, c.xkv)
        own = torch.arange(c.batch * self.cc, device=c._all.device, dtype=torch.int32) // self.cc
        c.rows, c.append = own.unsqueeze(1).repeat(1, c.max_len).contiguous(), False

    def __exit__(self, *exc):
        self.cache.rows, self.cache.append, self.cache.xkv = self.saved
        return False


class _IdeficsDecoder:
    """Model side of the search for Idefics: image states + per-token image mask + KV cache."""

    def __init__(self, engine: IdeficsEngine, pixel_values, image_attention_mask, batch, max_len, hooks, beams: int = 1):
        self.e, self.hooks = engine, hooks
        self.image_states = engine.encode_images(pixel_values)
        self.iam = image_attention_mask
        self.cache = KVCache(engine.arch, batch, max_len, engine.w.device, beams=beams)

    def _fwd(self, ids, am, iam):
        B, S = ids.shape
        return self.e.forward(input_ids=ids, attention_mask=am, image_states=self.image_states, image_attention_mask=iam,
                              kv_cache=self.cache, logits_rows=_last_rows(B, S, ids.device), **self.hooks)

    def prefill(self, ids, am):
        out = self._fwd(ids, am, self.iam)
        self.iam = self.iam[:, -1:, :]
        return out

    def step(self, new_ids, am):
        return self._fwd(new_ids, am, self.iam)

    def continuation(self, ids, am, cc, rows):
        """Logits rows `rows` of a continuation step on `cc` candidates per question: (B*cc, Tc) tokens behind the shared prompt.  Every
        token takes the image-mask row of the prompt's last token; a question's image states and cross-attention K|V are repeated."""
        Tc = ids.shape[1]
        rep = lambda t: t.repeat_interleave(cc, 0)
        with _shared_prompt(self.cache, cc):
            if self.cache.xkv is not None:
                self.cache.xkv = [rep(t) for t in self.cache.xkv]
            return self.e.forward(input_ids=ids, attention_mask=am, image_states=rep(self.image_states),
                                  image_attention_mask=rep(self.iam.expand(-1, Tc, -1)), kv_cache=self.cache, logits_rows=rows, **self.hooks)

    def replicate(self, nb):                       # HF prefills B*nb identical rows; replicate the prompt state instead
        self.cache.replicate(nb)
        if self.cache.xkv is not None:             # beams of one question share the image side: replicated once, never reordered
            self.cache.xkv = [t.repeat_interleave(nb, 0) for t in self.cache.xkv]
        self.image_states = self.image_states.repeat_interleave(nb, 0)
        self.iam = self.iam.repeat_interleave(nb, 0)

    def reorder(self, flat):
        self.cache.reorder(flat)

    def kv_rows(self):                             # the cache's row table (after replicate): licv_beam_step keeps it up to date itself
        return self.cache.rows

    def reorder_with_rows(self, flat, rows):
        self.cache.set_rows(rows)


class _Idefics2Decoder:
    """Idefics2: image hidden states only feed the prefill (they are scattered into the prompt embeddings); decode steps
    need the KV cache and HF's generate-time position ids (cumsum(mask)-1 with pads at 0, then previous+1 per step:
    transformers generation/utils.py:751-773, :975-985)."""

    def __init__(self, engine, pixel_values, pixel_attention_mask, batch, max_len, hooks, beams: int = 1):
        from .idefics2_engine import KVCache2
        self.e, self.hooks = engine, hooks
        self.img = engine.encode_images(pixel_values, pixel_attention_mask) if pixel_values is not None else None
        self.cache = KVCache2(engine.arch, batch, max_len, engine.w.device, beams=beams)
        self.pos = None

    def _fwd(self, ids, am, img):
        B, S = ids.shape
        return self.e.forward(input_ids=ids, attention_mask=am, image_hidden_states=img, position_ids=self.pos, kv_cache=self.cache,
                              logits_rows=_last_rows(B, S, ids.device), **self.hooks)

    def prefill(self, ids, am):
        self.pos = (am.long().cumsum(-1) - 1).masked_fill(am == 0, 0)
        out = self._fwd(ids, am, self.img)
        self.pos = self.pos[:, -1:]
        return out

    def step(self, new_ids, am):
        self.pos = self.pos + 1
        return self._fwd(new_ids, am, None)

    def continuation(self, ids, am, cc, rows):
        """As _IdeficsDecoder.continuation; the positions go on from the prompt's last one, as in a chain of decode steps."""
        Tc = ids.shape[1]
        pos = (self.pos + 1 + torch.arange(Tc, device=self.pos.device)).repeat_interleave(cc, 0)
        with _shared_prompt(self.cache, cc):
            return self.e.forward(input_ids=ids, attention_mask=am, image_hidden_states=None, position_ids=pos, kv_cache=self.cache,
                                  logits_rows=rows, **self.hooks)

    def replicate(self, nb):
        self.cache.replicate(nb)
        self.pos = self.pos.repeat_interleave(nb, 0)

    def reorder(self, flat):
        self.cache.reorder(flat)
        self.pos = self.pos.index_select(0, flat)

    def kv_rows(self):
        return self.cache.rows

    def reorder_with_rows(self, flat, rows):
        self.cache.set_rows(rows)
        self.pos = self.pos.index_select(0, flat)


@torch.no_grad()
def generate(engine: IdeficsEngine, input_ids: torch.Tensor, attention_mask: torch.Tensor, pixel_values: torch.Tensor,
             image_attention_mask: torch.Tensor, icv: Optional[torch.Tensor] = None,
             hook_layers: Optional[Sequence[int]] = None, max_new_tokens: int = 5, num_beams: int = 1, **kw) -> torch.Tensor:
    _precheck(engine.arch, num_beams, kw)
    hooks = dict(icv=icv, hook_layers=hook_layers) if icv is not None else {}
    model = _IdeficsDecoder(engine, pixel_values, image_attention_mask, input_ids.shape[0], input_ids.shape[1] + max_new_tokens, hooks, beams=num_beams)
    return _decode(model, engine.arch, input_ids, attention_mask, max_new_tokens=max_new_tokens, num_beams=num_beams, **kw)


@torch.no_grad()
def generate_idefics2(engine, input_ids: torch.Tensor, attention_mask: torch.Tensor, pixel_values: Optional[torch.Tensor] = None,
                      pixel_attention_mask: Optional[torch.Tensor] = None, icv: Optional[torch.Tensor] = None,
                      hook_layers: Optional[Sequence[int]] = None, max_new_tokens: int = 5, num_beams: int = 1, **kw) -> torch.Tensor:
    _precheck(engine.arch, num_beams, kw)
    hooks = dict(icv=icv, hook_layers=hook_layers) if icv is not None else {}
    model = _Idefics2Decoder(engine, pixel_values, pixel_attention_mask, input_ids.shape[0], input_ids.shape[1] + max_new_tokens, hooks, beams=num_beams)
    return _decode(model, engine.arch, input_ids, attention_mask, max_new_tokens=max_new_tokens, num_beams=num_beams, **kw)


@dataclass
class ContinuationScores:
    """token_logprobs (B, C, T) fp32: log p(candidate token | prompt, earlier candidate tokens), zero at padding; sum (B, C); mean (B, C):
    the sum divided by the candidate's length."""
    token_logprobs: torch.Tensor
    sum: torch.Tensor
    mean: torch.Tensor


# Rows (questions x candidates of a chunk) of one continuation pass.  Every pass streams all weights once whatever its row count, so
# a chunk should be large; 512 rows of a few tokens each are a few thousand GEMM rows, enough to amortise that stream, and bound the
# pass's scratch (rows x tokens x the hidden / MLP widths, and its logits rows x vocabulary) to that of a prefill of that many tokens.
DEFAULT_MAX_ROWS = 512


def _score(model, input_ids, attention_mask, candidates, candidate_lengths, max_rows) -> ContinuationScores:
    from . import ops
    from ._lib import APPEND_MAX_T
    dev = input_ids.device
    B, P = input_ids.shape
    if candidates.dim() != 3 or candidates.shape[0] != B or tuple(candidate_lengths.shape) != tuple(candidates.shape[:2]):
        raise ValueError(f"candidates must be (B, C, T) and candidate_lengths (B, C); got {tuple(candidates.shape)} and {tuple(candidate_lengths.shape)}")
    lens = candidate_lengths.to(device=dev, dtype=torch.long)
    C, T_in = candidates.shape[1:]
    lo, hi = int(lens.min()), int(lens.max())
    if lo < 1 or hi > T_in:
        raise ValueError(f"every candidate length must lie in [1, {T_in}]; got {lo} .. {hi}")
    if bool((attention_mask[:, -1] == 0).any()):
        raise ValueError("prompts must be left padded: the last column of attention_mask is masked for some row")
    T = hi                                                                 # columns that are padding for every candidate are dropped
    Tc = T - 1
    if Tc > APPEND_MAX_T:
        raise ValueError(f"candidates of {T} tokens need a continuation step of {Tc} tokens; the limit is LICV_APPEND_MAX_T = {APPEND_MAX_T}")
    if max_rows < B:
        raise ValueError(f"max_rows = {max_rows} is smaller than the batch of {B} prompts")
    tok_valid = torch.arange(T, device=dev)[None, None, :] < lens[:, :, None]                  # (B, C, T)
    cand = torch.where(tok_valid, candidates[:, :, :T].to(device=dev, dtype=torch.long), torch.zeros((), dtype=torch.long, device=dev))
    logits0 = model.prefill(input_ids, attention_mask)                    # (B, V): the prompt's last row, shared by a question's candidates
    V = logits0.shape[1]
    lp = torch.zeros((B, C, T), dtype=torch.float32, device=dev)
    first = ops.ce_rows(logits0, torch.arange(B, device=dev).repeat_interleave(C), cand[:, :, 0].reshape(-1), V)
    lp[:, :, 0] = -first.view(B, C)
    if Tc > 0:
        chunk = max(1, min(C, max_rows // B))
        for c0 in range(0, C, chunk):
            c1 = min(C, c0 + chunk)
            cc = c1 - c0
            ids = cand[:, c0:c1, :Tc].reshape(B * cc, Tc).contiguous()
            am = torch.cat([attention_mask.repeat_interleave(cc, 0), tok_valid[:, c0:c1, :Tc].reshape(B * cc, Tc).to(attention_mask.dtype)], 1)
            # flat row r * Tc + t predicts candidate token t + 1: the LM head runs on the rows whose target is a real token only
            sel = tok_valid[:, c0:c1, 1:].reshape(-1).nonzero().squeeze(1)
            if sel.numel() == 0:
                continue
            logits = model.continuation(ids, am, cc, sel)
            ce = ops.ce_rows(logits, torch.arange(sel.numel(), device=dev), cand[:, c0:c1, 1:].reshape(-1)[sel], V)
            flat = torch.zeros((B * cc * Tc,), dtype=torch.float32, device=dev)
            flat[sel] = -ce
            lp[:, c0:c1, 1:] = flat.view(B, cc, Tc)
    total = lp.sum(-1)
    return ContinuationScores(lp, total, total / lens.to(torch.float32))


@torch.no_grad()
def score_continuations(engine: IdeficsEngine, input_ids: torch.Tensor, attention_mask: torch.Tensor, pixel_values: torch.Tensor,
                        image_attention_mask: torch.Tensor, candidates: torch.Tensor, candidate_lengths: torch.Tensor,
                        icv: Optional[torch.Tensor] = None, hook_layers: Optional[Sequence[int]] = None,
                        max_rows: int = DEFAULT_MAX_ROWS) -> ContinuationScores:
    """Closed-set scoring under the hooked model: the log-likelihood of every candidate answer given its question's prompt.
    Model inputs as `generate` (prompts left padded); candidates (B, C, T) int64 right padded, candidate_lengths (B, C) >= 1.  One
    prefill on the B prompts; token 0 of every candidate is scored from the prompt's last row; tokens 1 .. T-1 from ONE continuation
    pass per chunk of candidates on tokens 0 .. T-2, which reads the prompt's KV cache through a row table (licv_append_attn) and
    appends nothing - no pass at all when every candidate is one token long.  The hook fires on every token.  max_rows bounds
    B * (candidates per chunk); see DEFAULT_MAX_ROWS."""
    hooks = dict(icv=icv, hook_layers=hook_layers) if icv is not None else {}
    T = candidates.shape[-1] if candidates.dim() == 3 else 1
    model = _IdeficsDecoder(engine, pixel_values, image_attention_mask, input_ids.shape[0], input_ids.shape[1] + max(T - 1, 1), hooks)
    return _score(model, input_ids, attention_mask, candidates, candidate_lengths, max_rows)


@torch.no_grad()
def score_continuations_idefics2(engine, input_ids: torch.Tensor, attention_mask: torch.Tensor, pixel_values: Optional[torch.Tensor] = None,
                                 pixel_attention_mask: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None,
                                 candidate_lengths: Optional[torch.Tensor] = None, icv: Optional[torch.Tensor] = None,
                                 hook_layers: Optional[Sequence[int]] = None, max_rows: int = DEFAULT_MAX_ROWS) -> ContinuationScores:
    """score_continuations for Idefics2 (model inputs as `generate_idefics2`)."""
    if candidates is None or candidate_lengths is None:
        raise ValueError("candidates and candidate_lengths are required")
    hooks = dict(icv=icv, hook_layers=hook_layers) if icv is not None else {}
    T = candidates.shape[-1] if candidates.dim() == 3 else 1
    model = _Idefics2Decoder(engine, pixel_values, pixel_attention_mask, input_ids.shape[0], input_ids.shape[1] + max(T - 1, 1), hooks)
    return _score(model, input_ids, attention_mask, candidates, candidate_lengths, max_rows)


def sample_params(temperature=None, top_k=None, top_p=None, min_p=None, seed=None):
    """The warpers of a sampled decode with transformers' defaults for what the caller leaves out (hf:generation/
    configuration_utils.py:616-618: temperature 1.0, top_k 50, top_p 1.0, min_p None) and the Philox key."""
    from . import _lib
    p = _lib.SampleParams()
    p.temperature = 1.0 if temperature is None else float(temperature)
    p.top_k = 50 if top_k is None else int(top_k)
    p.top_p = 1.0 if top_p is None else float(top_p)
    p.min_p = 0.0 if min_p is None else float(min_p)
    p.seed = (int(torch.randint(0, 2 ** 63 - 1, (1,)).item()) if seed is None else int(seed)) & (2 ** 64 - 1)
    return p


_CONSTRAINT_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens")
_BEAM_SAMPLE_CONSTRAINED = ("generate(do_sample=True, num_beams > 1) with repetition_penalty / no_repeat_ngram_size / bad_words_ids / "
                            "suppress_tokens / begin_suppress_tokens: beam-search multinomial sampling on processed log-probabilities "
                            "is not built on the native path")


def _vocab(a) -> int:
    return getattr(a, "total_vocab", None) or a.vocab_size


def check_constraints(vocab: int, repetition_penalty=None, no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None,
                      begin_suppress_tokens=None) -> bool:
    """The logits-processor keywords of `generate`, validated as transformers validates them (hf:generation/logits_process.py
    RepetitionPenaltyLogitsProcessor.__init__, NoRepeatNGramLogitsProcessor.__init__, NoBadWordsLogitsProcessor._validate_arguments;
    ids must also lie inside the vocabulary).  Returns whether any of them is on (off: None, penalty 1.0, size 0, an empty list)."""
    def is_int(t):
        return isinstance(t, int) and not isinstance(t, bool)

    if repetition_penalty is not None and (not isinstance(repetition_penalty, float) or not repetition_penalty > 0):
        raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty!r}")
    if no_repeat_ngram_size is not None and (not is_int(no_repeat_ngram_size) or no_repeat_ngram_size < 0):
        raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {no_repeat_ngram_size!r}")
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, (list, tuple)) or any(not isinstance(w, (list, tuple)) or len(w) == 0 for w in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists of token ids, but is {bad_words_ids!r}")
        if any(not is_int(t) or not 0 <= t < vocab for w in bad_words_ids for t in w):
            raise ValueError(f"each token of `bad_words_ids` has to be an integer in [0, {vocab}), but it is {bad_words_ids!r}")
    for name, lst in (("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens)):
        if lst is not None and (not isinstance(lst, (list, tuple)) or any(not is_int(t) or not 0 <= t < vocab for t in lst)):
            raise ValueError(f"`{name}` has to be a list of token ids in [0, {vocab}), but is {lst!r}")
    return bool((repetition_penalty or 1.0) != 1.0 or no_repeat_ngram_size or bad_words_ids or suppress_tokens or begin_suppress_tokens)


def _precheck(a, num_beams, kw):
    """Bad processor values and the one combination that is not built raise before the model side launches anything."""
    if check_constraints(_vocab(a), *(kw.get(k) for k in _CONSTRAINT_KEYS)) and kw.get("do_sample") and num_beams > 1:
        raise NotImplementedError(_BEAM_SAMPLE_CONSTRAINED)


def logits_constraints(device, vocab: int, eos: Optional[int], repetition_penalty=None, no_repeat_ngram_size=None, bad_words_ids=None,
                       suppress_tokens=None, begin_suppress_tokens=None):
    """The validated keywords as a licv.ops.LogitsConstraints with the lists on the device - or None when every one of them is
    off: the decode loop then launches and allocates nothing new."""
    if not check_constraints(vocab, repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens):
        return None
    from .ops import LogitsConstraints
    c = LogitsConstraints(device, 1.0 if repetition_penalty is None else repetition_penalty, no_repeat_ngram_size or 0, bad_words_ids,
                          suppress_tokens, begin_suppress_tokens, eos=eos)
    return c if c.active else None                                    # (the only bad word was [eos])


def _decode(model, a, input_ids: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int = 5, num_beams: int = 1,
            length_penalty: float = 1.0, min_new_tokens: int = 0, early_stopping=False,
            eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, do_sample: bool = False,
            temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
            min_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
            no_repeat_ngram_size: Optional[int] = None, bad_words_ids=None, suppress_tokens=None,
            begin_suppress_tokens=None) -> torch.Tensor:
    dev = input_ids.device
    sampling = sample_params(temperature, top_k, top_p, min_p, seed) if do_sample else None
    eos = a.eos_token_id if eos_token_id is None else eos_token_id
    # logits processors (csrc/logits_process.hip): None = all off, and then nothing below differs from the unconstrained decode
    cons = logits_constraints(dev, _vocab(a), eos, repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens,
                              begin_suppress_tokens)
    if cons is not None and sampling is not None and num_beams > 1:
        raise NotImplementedError(_BEAM_SAMPLE_CONSTRAINED)
    pad = a.pad_token_id if pad_token_id is None else pad_token_id
    B, P = input_ids.shape
    max_len = P + max_new_tokens
    nb = num_beams
    logits = model.prefill(input_ids, attention_mask)          # (B, V) rows in the model's dtype (a view with a padded row stride)

    def suppress_eos(lp, n_generated):
        if min_new_tokens > 0 and n_generated < min_new_tokens and eos is not None:
            lp = lp.clone()
            lp[..., eos] = -float("inf")
        return lp

    if nb == 1 and sampling is not None:                              # ---- multinomial sampling (_sample, do_sample): csrc/sample.hip
        state = SampleState(B, P, max_len, input_ids, eos, pad, min_new_tokens, sampling, constraints=cons)
        am = attention_mask
        while True:
            more = state.step(logits)                                 # one device -> host read per step
            if not more:
                break
            am = torch.cat([am, torch.ones((B, 1), dtype=am.dtype, device=dev)], 1)
            logits = model.step(state.next_tokens.view(B, 1), am)
        return state.result()

    if nb == 1:                                                       # ---- greedy (GenerationMixin._sample)
        seq = torch.full((B, max_len), pad, dtype=torch.long, device=dev)
        seq[:, :P] = input_ids
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        am = attention_mask
        cur = P
        buf = None
        while True:
            if cons is None:
                scores = logits.float()
            else:                                                     # hf _sample: the processors on the fp32 logits, history = seq[:, :cur]
                from .ops import logits_process
                buf = scores = logits_process(logits, seq, cur, P, cons, out=buf)
            scores = suppress_eos(scores, cur - P)
            nxt = scores.argmax(-1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            seq[:, cur] = nxt
            cur += 1
            if eos is not None:
                unfinished = unfinished & (nxt != eos)
            if cur >= max_len or not bool(unfinished.any()):
                break
            am = torch.cat([am, torch.ones((B, 1), dtype=am.dtype, device=dev)], 1)
            logits = model.step(nxt[:, None], am)
        return seq[:, :cur]

    # ---- beam search (GenerationMixin._beam_search, transformers 5.x): ONE kernel per step does the log-softmax, the top 2K
    # continuations per question and the whole bookkeeping (csrc/beam.hip; the torch restatement it replaced was ~60 launches a step)
    # hf:generation/utils.py:3319 — `output_fill_value = pad_token_id or eos_token_id[0]`: a pad id of 0 (Idefics' <unk>) is falsy
    # there, so finished beams are padded with EOS, not with the pad id (greedy above does use the pad id)
    fill = pad if (pad or eos is None) else eos
    # the prompt state is shared by a question's beams (HF prefills B*nb identical rows instead): no copy of the KV cache, only its row
    # table, which the search kernel then keeps up to date itself; the first step reads the B prefill rows directly
    model.replicate(nb)
    table = model.kv_rows() if hasattr(model, "kv_rows") and hasattr(model, "reorder_with_rows") else None
    search = BeamSearchState(B, nb, P, max_len, fill, input_ids, eos, length_penalty, early_stopping, min_new_tokens, kv_rows=table,
                             sampling=sampling, constraints=cons)
    am = attention_mask.repeat_interleave(nb, 0)
    first = True
    while True:
        unfinished = search.step(logits, shared_rows=first)            # one device -> host read per step (the loop's only sync point)
        first = False
        if not unfinished:
            break
        # reorder the per-beam model state (after the exit test: the last step's reorder would feed no further forward)
        if search.kv_rows is not None:
            model.reorder_with_rows(search.beam_src_flat, search.kv_rows)
        else:
            model.reorder(search.beam_src_flat)
        am = torch.cat([am, torch.ones((B * nb, 1), dtype=am.dtype, device=dev)], 1)
        logits = model.step(search.next_tokens.view(B * nb, 1), am)
    return search.result()


class BeamSearchState:
    """Device-side state of one beam search (running / finished token rows, scores, flags), advanced by `licv_beam_step`.
    Two copies of every buffer: the kernel gathers rows of the old state into the new one."""

    def __init__(self, B, nb, P, max_len, fill, input_ids, eos, length_penalty, early_stopping, min_new_tokens, kv_rows=None,
                 sampling=None, constraints=None):
        dev = input_ids.device
        # constraints: a licv.ops.LogitsConstraints (hf _beam_search: log_softmax, then the logits processors on every running beam's
        # history, then the search): licv_logits_process with normalize = 1 before each step, its rows into licv_beam_step as
        # final log-probabilities.  None = today's single call.
        assert constraints is None or sampling is None, "beam-search multinomial sampling with logits processors is not built"
        self.constraints, self._lp = constraints, None
        # sampling: a licv._lib.SampleParams (beam-search multinomial sampling through licv_beam_sample_step), None = beam search
        self.sampling = sampling
        self.B, self.nb, self.P, self.max_len, self.cur = B, nb, P, max_len, P
        self.eos = -1 if eos is None else int(eos)
        self.length_penalty, self.early_stopping, self.min_new_tokens = float(length_penalty), early_stopping is True, int(min_new_tokens)
        running = torch.full((B, nb, max_len), fill, dtype=torch.long, device=dev)
        running[:, :, :P] = input_ids[:, None, :]
        run_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        run_scores[:, 1:] = -1e9
        st = dict(running=running, finished=running.clone(), run_scores=run_scores,
                  fin_scores=torch.full((B, nb), -1e9, dtype=torch.float32, device=dev),
                  is_fin=torch.zeros((B, nb), dtype=torch.uint8, device=dev), improve=torch.ones((B,), dtype=torch.uint8, device=dev),
                  gen_len=torch.zeros((B, nb), dtype=torch.long, device=dev))
        self.state = [st, {k: torch.empty_like(v) for k, v in st.items()}]
        self.beam_src_flat = torch.empty((B * nb,), dtype=torch.long, device=dev)
        self.next_tokens = torch.empty((B * nb,), dtype=torch.long, device=dev)
        self.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.sync = torch.zeros((4,), dtype=torch.int32, device=dev)
        from . import _lib
        if sampling is None:
            self.scratch = torch.empty((int(_lib.lib().licv_beam_step_scratch_bytes(B, nb)),), dtype=torch.uint8, device=dev)
        else:                                                  # (holds an error counter that must start at zero)
            self.scratch = torch.zeros((int(_lib.lib().licv_beam_sample_scratch_bytes(B, nb)),), dtype=torch.uint8, device=dev)
        # optional: the KV cache's row table (B*nb, cache max_len) int32, ping-ponged like the rest of the state
        self.kv_rows = kv_rows
        self._kv_rows_next = torch.empty_like(kv_rows) if kv_rows is not None else None

    def step(self, logits: torch.Tensor, shared_rows: bool = False, logprobs_in: bool = False) -> bool:
        """logits: (B*nb, V) rows (bf16 or fp32, row stride = stride(0)); shared_rows: (B, V) rows of the prefill that all beams of a
        question share.  Returns whether the search continues (reads one int32 back).
        logprobs_in is a TEST HOOK (tests/test_beam_step_logprobs_gpu.py): the rows are fp32 final log-probabilities (-inf allowed)
        handed straight to licv_beam_step.  The product path never passes it - with `constraints` the pre-pass below makes such rows
        itself - so build nothing on it."""
        import ctypes as C
        from . import _lib
        from .ops import _dt, _p, _stream, check
        assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == (self.B if shared_rows else self.B * self.nb)
        a = _lib.BeamStepArgs()
        a.logits, a.logits_dtype, a.ld = logits.data_ptr(), _dt(logits), logits.stride(0)
        if self.constraints is not None:
            from .ops import logits_process
            if self._lp is None:
                self._lp = torch.empty((self.B * self.nb, logits.shape[1]), dtype=torch.float32, device=logits.device)
            running = self.state[0]["running"]                 # the state the previous step wrote: (B, nb, max_len)
            # first step: the B shared prefill rows, history = the prompt (all beams of a question hold it); later: every running beam
            hist, out = (running[:, 0, :], self._lp[:self.B]) if shared_rows else (running.view(self.B * self.nb, self.max_len), self._lp)
            logits_process(logits, hist, self.cur, self.P, self.constraints, normalize=True, out=out)
            a.logits, a.logits_dtype, a.ld = out.data_ptr(), _lib.LICV_F32_LOGPROBS, out.stride(0)
        if logprobs_in:
            assert logits.dtype == torch.float32 and self.constraints is None
            a.logits_dtype = _lib.LICV_F32_LOGPROBS
        a.q_stride_rows, a.beam_stride_rows = (1, 0) if shared_rows else (self.nb, 1)
        a.B, a.nb, a.V, a.max_len, a.cur, a.P = self.B, self.nb, logits.shape[1], self.max_len, self.cur, self.P
        a.eos = self.eos
        a.suppress_eos = 1 if (self.min_new_tokens > 0 and self.cur - self.P < self.min_new_tokens and self.eos >= 0) else 0
        a.length_penalty, a.early_stopping = self.length_penalty, 1 if self.early_stopping else 0
        src, dst = self.state
        for k in ("running", "finished", "run_scores", "fin_scores", "is_fin", "improve", "gen_len"):
            setattr(a, k + "_in", src[k].data_ptr())
            setattr(a, k + "_out", dst[k].data_ptr())
        a.beam_src_flat, a.next_tokens = self.beam_src_flat.data_ptr(), self.next_tokens.data_ptr()
        a.flags, a.sync = self.flags.data_ptr(), self.sync.data_ptr()
        a.scratch, a.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel()
        if self.kv_rows is not None:
            assert self.kv_rows.dtype == torch.int32 and self.kv_rows.is_contiguous() and self.kv_rows.shape[0] == self.B * self.nb
            a.kv_rows_in, a.kv_rows_out, a.kv_ld = self.kv_rows.data_ptr(), self._kv_rows_next.data_ptr(), self.kv_rows.shape[1]
        if self.sampling is None:
            check(_lib.lib().licv_beam_step(C.byref(a), _stream(logits)))
        else:
            check(_lib.lib().licv_beam_sample_step(C.byref(a), C.byref(self.sampling), _stream(logits)))
        if self.kv_rows is not None:
            self.kv_rows, self._kv_rows_next = self._kv_rows_next, self.kv_rows
        self.state = [dst, src]
        self.cur += 1
        f = int(self.flags[0])
        if f & 2:
            raise ValueError("beam-search sampling: a question has fewer than 2 * num_beams candidates of non-zero probability "
                             "(torch.multinomial raises here too); raise top_k / top_p or lower num_beams")
        return bool(f & 1)

    def result(self) -> torch.Tensor:
        st = self.state[0]
        out_len = self.P + int(st["gen_len"][:, 0].max())
        return st["finished"][:, 0, :out_len]


class SampleState:
    """Device-side state of multinomial sampling without beams (hf GenerationMixin._sample with do_sample=True), advanced by
    `licv_sample_step`: the running (B, max_len) id buffer, the unfinished flags and the loop flag."""

    def __init__(self, B, P, max_len, input_ids, eos, pad, min_new_tokens, sampling, constraints=None):
        dev = input_ids.device
        # constraints: a licv.ops.LogitsConstraints - hf _sample runs the logits processors on the fp32 logits before the warpers:
        # licv_logits_process (normalize = 0) into an fp32 buffer that licv_sample_step then reads (it ranks -inf correctly)
        self.constraints, self._lp = constraints, None
        self.B, self.P, self.max_len, self.cur = B, P, max_len, P
        self.eos = -1 if eos is None else int(eos)
        self.pad = int(pad) if pad is not None else (self.eos if self.eos >= 0 else 0)
        self.min_new_tokens, self.sampling = int(min_new_tokens), sampling
        self.seq = torch.full((B, max_len), self.pad, dtype=torch.long, device=dev)
        self.seq[:, :P] = input_ids
        self.unfinished = torch.ones((B,), dtype=torch.uint8, device=dev)
        self.next_tokens = torch.empty((B,), dtype=torch.long, device=dev)
        self.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.sync = torch.zeros((2,), dtype=torch.int32, device=dev)

    def step(self, logits: torch.Tensor) -> bool:
        """logits: (B, V) rows (bf16 or fp32, row stride = stride(0)).  Returns whether decoding continues (reads one int32 back)."""
        import ctypes as C
        from . import _lib
        from .ops import _dt, _stream, check
        assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == self.B
        if self.constraints is not None:
            from .ops import logits_process
            self._lp = logits = logits_process(logits, self.seq, self.cur, self.P, self.constraints, out=self._lp)
        a = _lib.SampleStepArgs()
        a.logits, a.logits_dtype, a.ld = logits.data_ptr(), _dt(logits), logits.stride(0)
        a.B, a.V = self.B, logits.shape[1]
        a.ids, a.ids_ld = self.seq.data_ptr(), self.seq.stride(0)
        a.max_len, a.cur, a.P = self.max_len, self.cur, self.P
        a.unfinished, a.next_tokens = self.unfinished.data_ptr(), self.next_tokens.data_ptr()
        a.eos, a.pad = self.eos, self.pad
        a.suppress_eos = 1 if (self.min_new_tokens > 0 and self.cur - self.P < self.min_new_tokens and self.eos >= 0) else 0
        a.flags, a.sync = self.flags.data_ptr(), self.sync.data_ptr()
        check(_lib.lib().licv_sample_step(C.byref(a), C.byref(self.sampling), _stream(logits)))
        self.cur += 1
        return bool(int(self.flags[0]))

    def result(self) -> torch.Tensor:
        return self.seq[:, :self.cur]
