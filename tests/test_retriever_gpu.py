"""RICE end to end on the GPU: MMTopkRetriever(mode="i2i") over synthetic images (PIL resize + crop on the host, licv_preprocess_images,
the CLIP tower, licv_topk_ip), its cache file, and the lists it returns driving icl_inference on the native tiny Idefics interface."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

import clip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_INDEX, SOURCES, NOISE_LEVELS = 24, [3, 17, 8, 0, 21, 12, 5, 9], 3


def pattern(seed, w=240, h=256):
    """A low-frequency colour pattern (random-init towers map unstructured noise images to nearly the same point)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = []
    for _ in range(3):
        f, ph, amp, base = rng.uniform(0.5, 3.0, 2), rng.uniform(0, 6.28, 2), rng.uniform(40, 100), rng.uniform(70, 180)
        ch.append(base + amp * np.sin(2 * np.pi * f[0] * xx / w + ph[0]) * np.cos(2 * np.pi * f[1] * yy / h + ph[1]))
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def perturbed(a, seed):
    rng = np.random.default_rng(seed)
    return np.clip(a.astype(np.int16) + rng.integers(-NOISE_LEVELS, NOISE_LEVELS + 1, a.shape), 0, 255).astype(np.uint8)


def tower():
    """A 4-layer tower at 224 x 224 / patch 32 whose value and output projections are scaled x 8: at the generators' 0.02 the class
    token (the only row the features read) barely hears the patches and every image lands within 1e-4 of the same point; at x 8 the
    restatement spreads the index images' cosines over [-0.97, 1]."""
    from licv.config import ClipVisionArch
    from licv.synthetic import synth_clip_vision_weights
    arch = ClipVisionArch(hidden_size=256, intermediate_size=1024, num_hidden_layers=4, num_attention_heads=4, image_size=224,
                          patch_size=32, projection_dim=128)
    sd = {k: v.float() for k, v in synth_clip_vision_weights(arch, 31, torch.bfloat16).items()}
    for k in sd:
        if k.endswith(("v_proj.weight", "out_proj.weight")):
            sd[k] *= 8.0
    return arch, {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def test_preprocess_kernel_with_clip_constants_returns_the_bf16_rounding_of_the_recorded_values(golden):
    from icv_src.utils.mm_topk_retriver import CLIP_MEAN, CLIP_STD, resize_center_crop_u8
    from licv import frontend
    g = golden("g18_clip_tiny")
    size = int(g["proc_size"])
    for i in range(int(g["n_images"])):
        u8 = resize_center_crop_u8(Image.fromarray(g[f"img_{i}"]), size)
        got = frontend.preprocess_images(torch.from_numpy(u8[None].copy()).to(DEV), mean=CLIP_MEAN, std=CLIP_STD)[0][0].float().cpu()
        want = torch.from_numpy(g[f"proc_{i}"]).to(torch.bfloat16).float()
        ulp = torch.ldexp(torch.ones(()), torch.frexp(want.abs().clamp_min(2.0 ** -120))[1] - 1 - 7)    # bf16: 8 significant bits
        d = (got - want).abs()
        print(f"image {i}: {float((got == want).float().mean()):.4f} bit-equal, worst {float((d / ulp).max()):.2f} bf16 ulp")
        assert (d <= ulp).all()


def test_rice_end_to_end(tmp_path, golden, monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import inference as I
    arch, sd = tower()
    index_u8 = [pattern(100 + i) for i in range(N_INDEX)]
    test_u8 = [perturbed(index_u8[s], 200 + j) for j, s in enumerate(SOURCES)]
    train_ds = [dict(image=Image.fromarray(a), question=f"tq{i}", answer=f"a{i}") for i, a in enumerate(index_u8)]
    val_ds = [dict(image=Image.fromarray(a), question=f"q{j}", question_id=j) for j, a in enumerate(test_u8)]

    # the generator's own condition, from the CPU restatement: the source ranks first with a margin above the bf16 noise
    cos = {}
    for dt in (torch.float32, torch.bfloat16):
        f = [R.clip_vision_forward(sd, arch, torch.from_numpy(R.clip_preprocess_ref([d["image"] for d in ds], 224)).to(torch.bfloat16).float(),
                                   dt)["features"].double() for ds in (val_ds, train_ds)]
        cos[dt] = f[0] @ f[1].T
    c = cos[torch.float32]
    rows = torch.arange(len(SOURCES))
    own = c[rows, SOURCES]
    other = c.clone()
    other[rows, SOURCES] = -2
    margin, noise = float((own - other.max(1).values).min()), float((cos[torch.bfloat16] - c).abs().max())
    print(f"restatement: smallest margin of the source over the best other image {margin:.3e}; its own bf16 run moves a cosine by at most {noise:.3e}")
    # ranking survives when the source's cosine drops by e and another's rises by e: margin > 2 e; 3 e asked of the generator
    assert margin >= 3 * noise, "generator: the perturbed copies are not separated from the other index images by 3 x the bf16 noise"

    cache = tmp_path / "rice_imgemb.pkl"
    r = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, index_field="image", mode="i2i", batch_size=8, num_workers=4,
                          cache_file=str(cache), device=DEV, clip_weights=(arch, sd))
    assert r.index_features.shape == (N_INDEX, arch.projection_dim) and r.test_features.shape == (len(SOURCES), arch.projection_dim)
    assert r.index_features.dtype == np.float32 and np.abs(np.linalg.norm(r.index_features.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    got_cos = torch.from_numpy(r.test_features).double() @ torch.from_numpy(r.index_features).double().T
    print(f"engine features: cosines within {float((got_cos - c).abs().max()):.3e} of the fp32 restatement")
    top1, top4 = r.retrieve(1), r.retrieve(4)
    assert top1 == [[s] for s in SOURCES]
    assert [row[0] for row in top4] == SOURCES and all(len(set(row)) == 4 for row in top4)

    # a second instance from the cache file: same lists, no tower
    import licv.clip_engine
    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", lambda *a, **k: pytest.fail("tower built although the cache file exists"))
    again = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, index_field="image", mode="i2i", cache_file=str(cache), device=DEV)
    assert again.retrieve(4) == top4 and again.retrieve(1) == top1
    rev = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, index_field="image", mode="i2i", cache_file=str(cache), device=DEV,
                            reversed_order=True)
    assert rev.retrieve(4) == [list(reversed(row)) for row in top4]

    # the lists drive icl_inference on the native tiny Idefics interface (fixture g5's token rows stand in for a tokenizer)
    from icv_src.icv_model.icv_intervention import LearnableICVInterventionLMM
    from licv.config import IDEFICS_TINY
    from licv.synthetic import synth_idefics_weights
    from lmm_icl_interface import IdeficsInterface
    from test_inference_tail import FakeTokenizer
    z = golden("g5_generate")
    larch = IDEFICS_TINY.with_(additional_vocab_size=0)
    lsd = synth_idefics_weights(larch, seed=21, dtype=torch.float32)
    lsd["model.embed_tokens.weight"] *= float(z["embed_scale"]); lsd["lm_head.weight"] *= float(z["head_scale"])
    model = LearnableICVInterventionLMM(IdeficsInterface(state_dict=lsd, arch=larch, device="cuda"), True, -1,
                                        "model.model.layers.<LAYER_NUM>", larch.num_layers)
    model.toggle_intervention(False)                                            # ref:inference.py:179, before the ICL baseline
    tok = FakeTokenizer()
    tok.special = {larch.pad_token_id, larch.bos_token_id, larch.eos_token_id}
    seen = []

    def prepare_input(prompts):
        seen.append(prompts)
        return {k: torch.from_numpy(z[f"left_in_{k}"])[: len(prompts)] for k in ("input_ids", "attention_mask", "pixel_values", "image_attention_mask")}

    proc = types.SimpleNamespace(tokenizer=tok, prepare_input=prepare_input)
    pm = types.SimpleNamespace(gen_query_text_without_label=lambda s: f"Question:{s['question']} Short answer:",
                               gen_ice_text_with_label=lambda s, add_sep_token=False: f"Question:{s['question']} Short answer:{s['answer']}")
    res = I.icl_inference(train_ds, val_ds, top4, model, pm, proc, bs=3, generate_kwargs=dict(max_new_tokens=4, num_beams=1, min_new_tokens=0))
    assert list(res) == list(range(len(SOURCES))) and all(isinstance(v["prediction"], str) and "image" not in v for v in res.values())
    assert seen[0][1][0] is train_ds[top4[1][0]]["image"] and seen[0][1][-2] is val_ds[1]["image"] and len(seen[0][0]) == 2 * 4 + 2
