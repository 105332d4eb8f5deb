"""The CLIP image tower on the GPU (licv/clip_engine.py) against the CPU restatement (tests/clip_ref.py), and the two row kernels
it adds to the library against torch ops."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ops():
    from licv import ops as o
    return o


def close_bf16(got, ref, ulps=1.0, exact_frac=0.99, scale_floor=None):
    """The criterion of tests/test_ops_gpu.py, restated: never more than `ulps` bf16 ulp off, at least `exact_frac` bit-equal."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    floor = ref.abs().max() * 2 ** -8 if scale_floor is None else scale_floor
    tol = ulps * (ref.abs() * 2 ** -7 + floor * 2 ** -1) * 1.001
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{int(bad.sum())} elements beyond {ulps} bf16 ulp; max diff {(got - ref).abs().max()}"
    if exact_frac:
        frac = float((got == ref).float().mean())
        print(f"bit-exact share {frac:.4f}")
        assert frac >= exact_frac, f"only {frac:.4f} of elements bit-exact"


def every_finite_bf16_in(lo, hi):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16)
    keep = torch.isfinite(v.float()) & (v.float() >= lo) & (v.float() <= hi)
    return v[keep]


def test_quick_gelu_matches_the_unfused_bf16_ops_on_every_value():
    x = every_finite_bf16_in(-12.0, 12.0)
    ref = x * torch.sigmoid(1.702 * x)
    assert ref.dtype == torch.bfloat16
    got = ops().quick_gelu(x.to(DEV).clone())
    close_bf16(got, ref, exact_frac=0.98)
    # a strided view: the padding columns come back untouched
    rows, dim, ld = 37, x.numel() // 37, x.numel() // 37 + 24
    buf = torch.full((rows, ld), 3.0, dtype=torch.bfloat16)
    buf[:, :dim] = x[:rows * dim].view(rows, dim)
    dev = buf.to(DEV)
    ops().quick_gelu(dev, rows=rows, dim=dim, ld=ld)
    out = dev.cpu()
    assert (out[:, dim:] == 3.0).all()
    close_bf16(out[:, :dim], ref[:rows * dim].view(rows, dim), exact_frac=0.98)


def _ulp32(ref64):
    a = np.abs(ref64).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(5, 32), (300, 512), (17, 768), (3, 1000)])
def test_l2_normalize_rows(dt, shape):
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(3)) * 3).to(dt)
    got = ops().l2_normalize_rows(x.to(DEV)).cpu()
    assert got.dtype == torch.float32 and got.shape == x.shape
    x64 = x.double().numpy()
    ref = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
    err = np.abs(got.numpy().astype(np.float64) - ref) / _ulp32(ref)
    norms = np.linalg.norm(got.numpy().astype(np.float64), axis=1)
    print(f"l2_normalize {dt} {shape}: worst {err.max():.2f} fp32 ulp, norms within {np.abs(norms - 1).max():.2e} of 1")
    assert err.max() <= 2.0
    assert np.abs(norms - 1).max() <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------ the tower
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _judge(what, hip_embeds, hip_feats, ref32, ref16):
    """As tests/test_fullwidth_gpu.py judges the engines: no further from the fp32 restatement than 1.25 x the restatement's own bf16
    run is, plus 1e-3."""
    r_hip, r_ref = _rel(hip_embeds.float(), ref32["image_embeds"]), _rel(ref16["image_embeds"].float(), ref32["image_embeds"])
    cos = lambda f: float((1 - (f.double().cpu() * ref32["features"].double()).sum(-1)).max())
    c_hip, c_ref = cos(hip_feats), cos(ref16["features"])
    print(f"{what}: image_embeds relative L2 vs fp32: engine {r_hip:.3e}, restatement bf16 {r_ref:.3e}; "
          f"worst 1 - cosine of the unit features: engine {c_hip:.3e}, restatement bf16 {c_ref:.3e}")
    assert torch.isfinite(hip_embeds.float()).all() and torch.isfinite(hip_feats).all()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: engine {r_hip:.3e} vs restatement bf16 {r_ref:.3e}"
    assert c_hip <= 1.25 * c_ref + 1e-3, f"{what}: engine {c_hip:.3e} vs restatement bf16 {c_ref:.3e}"


def test_toy_tower_against_the_transformers_fixture(golden):
    import clip_ref as R
    from licv.clip_engine import ClipVisionEngine
    g = golden("g18_clip_tiny")
    arch, sd, pix = R.load_g18(g)
    eng = ClipVisionEngine(arch, sd, DEV)
    hidden = []
    embeds = eng.image_embeds(pix.to(DEV), hidden_states=hidden)
    feats = eng.encode(pix.to(DEV))
    assert feats.dtype == torch.float32 and feats.shape == (pix.shape[0], arch.projection_dim) and feats.is_cuda
    ref32 = dict(image_embeds=torch.from_numpy(g["image_embeds"]), features=torch.from_numpy(g["features"]))
    ref16 = R.clip_vision_forward(sd, arch, pix, dtype=torch.bfloat16)
    for i, h in enumerate(hidden):
        r_hip, r_ref = _rel(h.float(), torch.from_numpy(g[f"hidden_{i}"])), _rel(ref16["hidden_states"][i].float(), torch.from_numpy(g[f"hidden_{i}"]))
        print(f"hidden state {i}: engine {r_hip:.3e}, restatement bf16 {r_ref:.3e}")
        assert r_hip <= 1.25 * r_ref + 1e-3
    _judge("toy tower", embeds, feats, ref32, ref16)
    norms = feats.double().norm(dim=-1).cpu()
    assert (norms - 1).abs().max() <= 2.0 ** -22


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_full_width_tower_against_the_restatement(act):
    import clip_ref as R
    from licv.clip_engine import ClipVisionEngine
    from licv.config import CLIP_VIT_B32
    from licv.synthetic import synth_clip_vision_weights, trained_like_
    from dataclasses import replace
    arch = replace(CLIP_VIT_B32, hidden_act=act)
    n = 64 if act == "quick_gelu" else 16
    sd = trained_like_(synth_clip_vision_weights(arch, seed=21, dtype=torch.bfloat16), arch.num_hidden_layers)
    sd = {k: v.float() for k, v in sd.items()}
    pix = torch.randn(n, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(22)).to(torch.bfloat16).float()
    eng = ClipVisionEngine(arch, sd, DEV)
    embeds = eng.image_embeds(pix.to(DEV))
    feats = eng.encode(pix.to(DEV))
    ref32 = R.clip_vision_forward(sd, arch, pix, dtype=torch.float32)
    ref16 = R.clip_vision_forward(sd, arch, pix, dtype=torch.bfloat16)
    _judge(f"ViT-B/32 width, {act}, n = {n}", embeds, feats, ref32, ref16)
