"""Mirror of the hot-path functions of the reference's `inference.py` (ref:inference.py:206-211, 246-377): `generate_answers` — ICV
scaling, hooked generate, prompt strip, `batch_decode` — the `icv_inference` batching loop around it, and the ICL baseline's
`icl_inference` (few-shot prompts whose demonstrations come from `ice_idx_list`: drawn at random, `random_ice_idx_list`, or by RICE,
`icv_src.utils.mm_topk_retriver.MMTopkRetriever`), on the native interfaces.  The Hydra `main` and dataset loading are out of scope
(SURVEY.md §2 rows 13-14); a maintainer who runs the reference's own `inference.py` against this package
(`PYTHONPATH=licv-vqa_amd`) gets the same functions from the reference file itself, driving the same
`LearnableICVInterventionLMM.generate` and the same retriever class."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import torch


@torch.inference_mode()
def generate_answers(inputs, model, processor, generate_kwargs, in_context_vector=None, alpha=None) -> List[str]:
    """ref:inference.py:299-321.  `model` = LearnableICVInterventionLMM; `inputs` as `processor.prepare_input` returns them
    (already on the device).  The vector handed to the hooks is alpha[..., None] * in_context_vector (1, L, H); the first
    `attention_mask.shape[1]` ids of every returned row are the (padded) prompt and are dropped before decoding."""
    icv = None
    if in_context_vector is not None:
        icv = alpha.unsqueeze(dim=-1) * in_context_vector
    out = model.generate(**inputs, **generate_kwargs, icv=icv)
    n_prompt = int(inputs["attention_mask"].shape[1])
    rows = out.tolist()
    return processor.tokenizer.batch_decode([r[n_prompt:] for r in rows], skip_special_tokens=True)


def _chunks(it: Iterable, n: int):
    buf = []
    for x in it:
        buf.append(x)
        if len(buf) == n:
            yield buf
            buf = []
    if buf:
        yield buf


@torch.inference_mode()
def icv_inference(val_ds: Sequence[dict], icv_model, prompt_manager, processor, bs: int, generate_kwargs: dict,
                  instruction: str = "", in_context_vector: Optional[torch.Tensor] = None,
                  alpha: Optional[torch.Tensor] = None) -> Dict[int, dict]:
    """ref:inference.py:246-297: zero-shot prompts [instruction?, image, "Question: ... Short answer:"] in chunks of `bs`,
    hooked generate, one result record per sample ({"prediction": text, **sample without its image}).  As in the reference a
    short LAST chunk is still `bs` prompts wide (the trailing ones carry the instruction only) and only the first
    len(batch) generations are kept."""
    results: Dict[int, dict] = {}
    index = 0
    for batch in _chunks(val_ds, bs):
        prompts = [[instruction] if instruction else [] for _ in range(bs)]
        for i, sample in enumerate(batch):
            prompts[i].extend([sample["image"], prompt_manager.gen_query_text_without_label(sample)])
        query_inputs = processor.prepare_input(prompts)
        query_inputs = {k: v.to(icv_model.lmm.device) for k, v in query_inputs.items()}
        generated = generate_answers(inputs=query_inputs, model=icv_model, processor=processor, generate_kwargs=generate_kwargs,
                                     in_context_vector=in_context_vector, alpha=alpha)
        for i in range(len(batch)):
            rec = dict(batch[i])
            rec.pop("image")
            results[index] = {"prediction": generated[i], **rec}
            index += 1
    return results


def random_ice_idx_list(n_train: int, n_val: int, shot_num: int, rng=None) -> List[List[int]]:
    """ref:inference.py:206-211, the branch without RICE: for every test sample `shot_num` distinct training indices drawn without
    replacement.  `rng`: a `random.Random` (default: the module-level generator, as the reference uses it)."""
    import random
    rng = random if rng is None else rng
    pool = list(range(n_train))
    return [rng.sample(pool, shot_num) for _ in range(n_val)]


@torch.inference_mode()
def icl_inference(train_ds: Sequence[dict], val_ds: Sequence[dict], ice_idx_list: Sequence[Sequence[int]], model, prompt_manager,
                  processor, bs: int, generate_kwargs: dict, instruction: str = "") -> Dict[int, dict]:
    """ref:inference.py:323-377, the in-context-learning baseline: prompts [instruction?, (ice image, ice text with label) x shots,
    query image, "Question: ... Short answer:"] with the demonstrations of sample i taken from train_ds in the order of
    ice_idx_list[i], in chunks of `bs`, plain generate (no vector: the hooks get icv=None), one result record per sample.  As in
    `icv_inference` a short last chunk is still `bs` prompts wide and the caller's samples are not mutated."""
    results: Dict[int, dict] = {}
    index = 0
    for batch in _chunks(val_ds, bs):
        prompts = [[instruction] if instruction else [] for _ in range(bs)]
        sub_ice_idx_list = ice_idx_list[index:index + bs]
        for i, sample in enumerate(batch):
            for ice_idx in sub_ice_idx_list[i]:
                ice = train_ds[int(ice_idx)]
                prompts[i].extend([ice["image"], prompt_manager.gen_ice_text_with_label(ice, add_sep_token=True)])
            prompts[i].extend([sample["image"], prompt_manager.gen_query_text_without_label(sample)])
        inputs = processor.prepare_input(prompts)
        inputs = {k: v.to(model.lmm.device) for k, v in inputs.items()}
        generated = generate_answers(inputs=inputs, model=model, processor=processor, generate_kwargs=generate_kwargs)
        for i in range(len(batch)):
            rec = dict(batch[i])
            rec.pop("image")
            results[index] = {"prediction": generated[i], **rec}
            index += 1
    return results


def _tokenize_candidates(processor, texts: Sequence[Sequence[str]]):
    """texts[b][c] -> (ids (B, C, T) int64 right padded with 0, lengths (B, C)); every question must offer the same number of candidates."""
    C = len(texts[0])
    if C == 0 or any(len(t) != C for t in texts):
        raise ValueError("every sample must offer the same, non-zero number of candidates")
    toks = [[list(processor.tokenizer(text, add_special_tokens=False)["input_ids"]) for text in row] for row in texts]
    if any(len(t) == 0 for row in toks for t in row):
        raise ValueError("a candidate tokenised to nothing")
    T = max(len(t) for row in toks for t in row)
    ids = torch.zeros((len(texts), C, T), dtype=torch.long)
    lengths = torch.zeros((len(texts), C), dtype=torch.long)
    for b, row in enumerate(toks):
        for c, t in enumerate(row):
            ids[b, c, :len(t)] = torch.tensor(t, dtype=torch.long)
            lengths[b, c] = len(t)
    return ids, lengths


@torch.inference_mode()
def rank_answers(inputs, model, processor, candidates: Sequence[Sequence[str]], in_context_vector=None, alpha=None, normalize: str = "sum"):
    """Closed-set counterpart of `generate_answers`: ranks candidates[b] (a list of strings per prompt row of `inputs`, or one list of
    strings offered to every row) by their
    log-likelihood under the hooked model (`model.score_candidates`), summed over the candidate's tokens (normalize="sum") or divided
    by their number ("mean").  The text is tokenised as given, `processor.tokenizer(text, add_special_tokens=False)`: whether a
    candidate starts with a space is the caller's choice.  The vector handed to the hooks is alpha[..., None] * in_context_vector.
    Returns (index of the best candidate per row, scores per row as lists of floats)."""
    if normalize not in ("sum", "mean"):
        raise ValueError(f"normalize must be 'sum' or 'mean', not {normalize!r}")
    icv = None
    if in_context_vector is not None:
        icv = alpha.unsqueeze(dim=-1) * in_context_vector
    if len(candidates) and isinstance(candidates[0], str):               # one list for every prompt row
        candidates = [list(candidates)] * int(inputs["input_ids"].shape[0])
    ids, lengths = _tokenize_candidates(processor, candidates)
    dev = inputs["input_ids"].device
    out = model.score_candidates(**inputs, candidates=ids.to(dev), candidate_lengths=lengths.to(dev), icv=icv)
    scores = getattr(out, normalize)
    return scores.argmax(-1).tolist(), scores.tolist()


@torch.inference_mode()
def rank_inference(val_ds: Sequence[dict], icv_model, prompt_manager, processor, bs: int, candidates, instruction: str = "",
                   in_context_vector: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
                   normalize: str = "sum") -> Dict[int, dict]:
    """`icv_inference` with candidate ranking in place of generation: the same zero-shot prompts in chunks of `bs`, one result record
    per sample: {"prediction": text of the best candidate, "scores": [score of every candidate], **sample without its image}.
    candidates: a list of strings offered to every sample, or the name of a sample field that holds that sample's list (all lists
    equally long).  Candidates are tokenised as given (see `rank_answers`).  As in `icv_inference` a short last chunk is still `bs`
    prompts wide (the trailing prompts are scored against the first sample's candidates and dropped) and the samples are not mutated."""
    results: Dict[int, dict] = {}
    index = 0
    for batch in _chunks(val_ds, bs):
        prompts = [[instruction] if instruction else [] for _ in range(bs)]
        for i, sample in enumerate(batch):
            prompts[i].extend([sample["image"], prompt_manager.gen_query_text_without_label(sample)])
        per_sample = [list(s[candidates]) if isinstance(candidates, str) else list(candidates) for s in batch]
        per_sample += [per_sample[0]] * (bs - len(batch))
        query_inputs = processor.prepare_input(prompts)
        query_inputs = {k: v.to(icv_model.lmm.device) for k, v in query_inputs.items()}
        best, scores = rank_answers(inputs=query_inputs, model=icv_model, processor=processor, candidates=per_sample,
                                    in_context_vector=in_context_vector, alpha=alpha, normalize=normalize)
        for i in range(len(batch)):
            rec = dict(batch[i])
            rec.pop("image")
            results[index] = {"prediction": per_sample[i][best[i]], "scores": scores[i], **rec}
            index += 1
    return results
