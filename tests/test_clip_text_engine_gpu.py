"""The CLIP text tower on the GPU (licv/clip_engine.py ClipTextEngine: packed tokens) against the transformers fixture g19 and the CPU
restatement on the padded batch (tests/clip_text_ref.py)."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import clip_text_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _judge(what, hip, ref16, ref32):
    """The rule of tests/test_clip_engine_gpu.py::_judge: no further from the fp32 values than 1.25 x the restatement's own bf16 run is,
    plus 1e-3 (relative L2)."""
    r_hip, r_ref = _rel(hip.float(), ref32), _rel(ref16.float(), ref32)
    print(f"{what}: relative L2 vs fp32: engine {r_hip:.3e}, restatement bf16 {r_ref:.3e}")
    assert torch.isfinite(hip.float()).all()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: engine {r_hip:.3e} vs restatement bf16 {r_ref:.3e}"


def _judge_features(what, hip_feats, ref16_feats, ref32_feats):
    cos = lambda f: float((1 - (f.double().cpu() * ref32_feats.double()).sum(-1)).max())
    c_hip, c_ref = cos(hip_feats), cos(ref16_feats)
    print(f"{what}: worst 1 - cosine of the unit features: engine {c_hip:.3e}, restatement bf16 {c_ref:.3e}")
    assert c_hip <= 1.25 * c_ref + 1e-3, f"{what}: engine {c_hip:.3e} vs restatement bf16 {c_ref:.3e}"
    norms = hip_feats.double().norm(dim=-1).cpu()
    assert (norms - 1).abs().max() <= 2.0 ** -22


@pytest.mark.parametrize("eos", [2, 95])
def test_toy_tower_against_the_transformers_fixture(golden, eos):
    from licv.clip_engine import ClipTextEngine
    arch, sd, ids, mask, want = R.load_g19(golden("g19_clip_text_tiny"), eos)
    eng = ClipTextEngine(arch, sd, DEV)
    hidden = []
    embeds = eng.text_embeds(ids, mask, hidden_states=hidden)
    feats = eng.encode(ids, mask)
    assert embeds.dtype == torch.bfloat16 and embeds.shape == (ids.shape[0], arch.projection_dim)
    assert feats.dtype == torch.float32 and feats.shape == (ids.shape[0], arch.projection_dim) and feats.is_cuda
    ref16 = R.clip_text_forward(sd, arch, ids, mask, dtype=torch.bfloat16)
    assert len(hidden) == arch.num_hidden_layers + 1
    for i, h in enumerate(hidden):
        assert h.shape == want[f"hidden_{i}"].shape                    # packed: one row per valid token
        _judge(f"hidden state {i}", h, R.valid_rows(ref16["hidden_states"][i], mask), want[f"hidden_{i}"])
    _judge(f"text_embeds (eos_token_id {eos})", embeds, ref16["text_embeds"], want["text_embeds"])
    _judge_features(f"features (eos_token_id {eos})", feats, ref16["features"], want["features"])


@functools.lru_cache(maxsize=None)
def _full_width_batch():
    from licv.config import CLIP_TEXT_B32 as A
    rng = np.random.default_rng(23)
    lens = rng.integers(3, 78, 64)
    lens[:2] = (3, 77)
    S = int(lens.max())
    ids = np.full((64, S), A.vocab_size - 1, dtype=np.int64)             # pad id = eos id = the largest id, as the public tokenizer has it
    mask = np.zeros((64, S), dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(3, A.vocab_size - 2, n)
        ids[i, 0], ids[i, n - 1] = A.vocab_size - 2, A.vocab_size - 1
        mask[i, :n] = 1
    return torch.from_numpy(ids), torch.from_numpy(mask)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_full_width_tower_against_the_restatement(act):
    from licv.clip_engine import ClipTextEngine
    from licv.config import CLIP_TEXT_B32
    from licv.synthetic import synth_clip_text_weights, trained_like_
    arch = replace(CLIP_TEXT_B32, hidden_act=act)
    sd = trained_like_(synth_clip_text_weights(arch, seed=24, dtype=torch.bfloat16), arch.num_hidden_layers)
    sd = {k: v.float() for k, v in sd.items()}
    ids, mask = _full_width_batch()
    eng = ClipTextEngine(arch, sd, DEV)
    embeds = eng.text_embeds(ids, mask)
    feats = eng.encode(ids, mask)
    ref32 = R.clip_text_forward(sd, arch, ids, mask, dtype=torch.float32)
    ref16 = R.clip_text_forward(sd, arch, ids, mask, dtype=torch.bfloat16)
    _judge(f"B/32 text width, {act}: text_embeds", embeds, ref16["text_embeds"], ref32["text_embeds"])
    _judge_features(f"B/32 text width, {act}: features", feats, ref16["features"], ref32["features"])
