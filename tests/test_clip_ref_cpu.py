"""The CPU restatements of tests/clip_ref.py against what the installed transformers wrote into g18 (tools/make_golden_clip.py): the
CLIP image tower with projection, and CLIPImageProcessor."""
import numpy as np
import torch

import clip_ref as R


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def test_tower_matches_transformers_in_fp32(golden):
    g = golden("g18_clip_tiny")
    arch, sd, pix = R.load_g18(g)
    assert arch.hidden_act == "quick_gelu" and arch.tokens == 5
    out = R.clip_vision_forward(sd, arch, pix, dtype=torch.float32)
    assert len(out["hidden_states"]) == arch.num_hidden_layers + 1
    for i, h in enumerate(out["hidden_states"]):
        e = rel(h, g[f"hidden_{i}"])
        print(f"hidden state {i}: relative L2 {e:.2e}")
        assert e <= 1e-5
    e = rel(out["image_embeds"], g["image_embeds"])
    print(f"image_embeds: relative L2 {e:.2e}")
    assert e <= 1e-5
    assert rel(out["features"], g["features"]) <= 1e-5


def test_tower_in_bf16_stays_near_its_fp32_run(golden):
    g = golden("g18_clip_tiny")
    arch, sd, pix = R.load_g18(g)
    out = R.clip_vision_forward(sd, arch, pix, dtype=torch.bfloat16)
    assert out["image_embeds"].dtype == torch.bfloat16 and out["features"].dtype == torch.float32
    # a sanity bound, not a parity bar: 2 layers of bf16 ops, each within 2^-8 relative, leave a few ulp; 8 x 2^-8 is ample
    assert rel(out["image_embeds"].float(), g["image_embeds"]) <= 8 * 2 ** -8


def test_arch_reads_both_config_layouts_and_refuses_other_activations():
    import pytest
    from licv.config import ClipVisionArch
    vis = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, image_size=64, patch_size=32,
               layer_norm_eps=1e-5, hidden_act="gelu")
    a = ClipVisionArch.from_hf(dict(vis, projection_dim=32))
    b = ClipVisionArch.from_hf({"vision_config": vis, "text_config": {}, "projection_dim": 32})
    assert a == b and a.hidden_act == "gelu" and a.head_dim == 16
    with pytest.raises(ValueError, match="hidden_act"):
        ClipVisionArch.from_hf(dict(vis, projection_dim=32, hidden_act="relu"))
    with pytest.raises(KeyError, match="projection_dim"):
        ClipVisionArch.from_hf(vis)


def test_image_preprocessing_restatement_equals_the_recorded_processor_outputs(golden):
    from PIL import Image
    g = golden("g18_clip_tiny")
    size = int(g["proc_size"])
    for i in range(int(g["n_images"])):
        img = Image.fromarray(g[f"img_{i}"])
        got = R.clip_preprocess_ref([img], size)[0]
        want = g[f"proc_{i}"]
        assert got.shape == want.shape == (3, size, size) and got.dtype == np.float32
        ulp = np.nextafter(np.abs(want), np.float32(np.inf)) - np.abs(want)
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"image {i} {img.size} {img.mode}: max difference {d.max():.3e}")
        assert (d <= ulp).all()
