"""Hooked generate behind a LONG left padding, against the reference's own bf16 decode (fixture g16_generate_idefics2_bf16_stable:
every row reproduced by 72 re-runs of the reference jittered by +-1 bf16 ulp; tests/test_generate_bf16_gpu.py holds the engine to it
at the fixture's own length, 20 tokens).  The 16 `left` prompts are left-padded - input_ids with the pad id the fixture already has
under its masked positions, attention_mask with 0 - to a total length P.  Position ids come from the mask, so nothing the reference
computes on the visible tokens changes, and generate(...)[:, P:] must equal the fixture's new tokens: beam search (3 beams, 5 tokens,
length_penalty 0), greedy, and greedy with the hook off, 48 rows in all.

(a) P = 200 under ops.decode_split(min_keys=1, n_splits=3): every decode step of the Idefics2 engine takes the split-key kernels,
    behind the beam search's row table.  201 .. 205 keys are four 64-key sweeps; three splits asked for come out as two of two
    sweeps each (no split is left empty), the first of them - keys 0 .. 127, all padding - wholly masked in every row.
(b) P = 10 300 with the default settings: past + 1 > 10 240 keys, the route chosen automatically; before licv_decode_attn_split the
    first decode step stopped with "history of 10301 keys exceeds the kernel's LDS budget".

Rows excluded: none.  The record: the same prompts padded to P = 10 000, where licv_decode_attn - the single launch,
untouched here - serves every decode step, return 48 of 48 rows of the fixture, so the padding does not disturb the prefill and no
row needs an exemption (at most 2 of 48 would have been allowed)."""
import functools

import pytest
import torch

from licv.config import IDEFICS2_TINY
from licv.synthetic import synth_idefics2_weights

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
EXCLUDED = ()            # (tag, row) pairs that differ at P = 10 000 through the single launch already: none (see above)


@functools.lru_cache(maxsize=None)
def _wrapper(weights_seed, embed_scale, head_scale, down_scale):
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from lmm_icl_interface import Idefics2Interface
    arch = IDEFICS2_TINY
    sd = synth_idefics2_weights(arch, seed=weights_seed, dtype=torch.float32)
    sd["model.text_model.embed_tokens.weight"] *= embed_scale
    sd["lm_head.weight"] *= head_scale
    for l in range(arch.num_layers):
        sd[f"model.text_model.layers.{l}.mlp.down_proj.weight"] *= down_scale
    iface = Idefics2Interface(state_dict=sd, arch=arch, device=DEV, max_positions=10368)
    return LearnableICVInterventionLMM(iface, True, -1, "model.model.text_model.layers.<LAYER_NUM>.mlp", arch.num_layers)


def _padded_batch(z, P):
    ids, mask = T(z["left_in_input_ids"]), T(z["left_in_attention_mask"])
    pad_ids = set(ids[mask == 0].tolist())
    assert len(pad_ids) == 1, "the fixture's masked positions hold one pad id"
    B, S = ids.shape
    batch = {"input_ids": torch.cat([torch.full((B, P - S), pad_ids.pop(), dtype=ids.dtype), ids], 1),
             "attention_mask": torch.cat([torch.zeros((B, P - S), dtype=mask.dtype), mask], 1),
             "pixel_values": T(z["left_in_pixel_values"]), "pixel_attention_mask": T(z["left_in_pixel_attention_mask"])}
    return {k: v.to(DEV) for k, v in batch.items()}, S


def _check(z, P):
    w = _wrapper(int(z["weights_seed"]), float(z["embed_scale"]), float(z["head_scale"]), float(z["down_scale"]))
    icv = T(z["icv"]).to(DEV)
    batch, S = _padded_batch(z, P)
    kw = dict(max_new_tokens=5, length_penalty=0.0, min_new_tokens=0)
    got = {"beam": w.generate(icv=icv, **batch, num_beams=3, **kw).cpu(), "greedy": w.generate(icv=icv, **batch, num_beams=1, **kw).cpu()}
    w.toggle_intervention(False)
    try:
        got["greedy_off"] = w.generate(icv=icv, **batch, num_beams=1, **kw).cpu()
    finally:
        w.toggle_intervention(True)
    bad, total = [], 0
    for tag, ids in got.items():
        gold = T(z[f"left_bf16_{tag}_ids"])[:, S:]
        assert ids.shape == (gold.shape[0], P + gold.shape[1]), (tag, ids.shape)
        same = (ids[:, P:] == gold).all(dim=1)
        for r in range(len(same)):
            if (tag, r) in EXCLUDED:
                continue
            total += 1
            if not bool(same[r]):
                bad.append((tag, r))
        print(f"\n  P={P} {tag}: {int(same.sum())}/{len(same)} rows identical to the reference's bf16 decode")
    assert len(EXCLUDED) <= 2 and total == 48 - len(EXCLUDED)
    assert not bad, f"P={P}: rows that differ from the reference's bf16 decode: {bad}"


def test_forced_split_route_behind_a_short_padding(golden):
    from licv import ops
    before = ops.decode_split_settings()
    with ops.decode_split(min_keys=1, n_splits=3):
        assert ops.decode_split_settings() == (1, 3)
        _check(golden("g16_generate_idefics2_bf16_stable"), 200)
    assert ops.decode_split_settings() == before == (10241, None)


def test_automatic_route_beyond_10240_keys(golden):
    from licv import ops
    assert ops.decode_split_settings() == (10241, None)
    _check(golden("g16_generate_idefics2_bf16_stable"), 10300)
