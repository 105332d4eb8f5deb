"""The register-direct GEMM epilogues (flow64: select 60, flow: select 20) after their instruction-level rewrite: pair-wise bf16
packing, block-wise erf-GELU (one tail test per lane block of eight values), residual add on the pairs as loaded, pair-wise rounding
in SwiGLU.  None of it moves a rounding point, so every check here is bit for bit."""
import hashlib
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_epilogue_digests.json"
VARIANTS = ["plain", "bias", "bias_gelu", "bias_gelu_tanh", "bias_relu", "swiglu", "bias_res_bf16", "res_bf16_inplace"]
GELU_ZM = 2.2                       # csrc/gemm_common.h: z = x / sqrt 2 below -2.2 takes the erfcx tail


def ops():
    from licv import ops as _ops
    return _ops


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def run_selects(fn, selects):
    from licv import _lib
    outs = {}
    try:
        for sel in selects:
            _lib.lib().licv_gemm_select(sel)
            outs[sel] = fn()
    finally:
        _lib.lib().licv_gemm_select(0)
    return outs


def bits(t):
    return t.contiguous().view(torch.int16)


def variant_output(variant, a, w, bias, res):
    """One epilogue variant of test_gemm_flow64_kernel_matches_general_kernel (tests/test_ops_gpu.py), same keyword forms."""
    kw = {}
    if variant.startswith("bias"):
        kw["bias"] = bias
    if variant.endswith("gelu"):
        kw["act"] = "gelu"
    elif variant.endswith("gelu_tanh"):
        kw["act"] = "gelu_tanh"
    elif variant.endswith("relu"):
        kw["act"] = "relu"
    elif variant == "swiglu":
        kw["swiglu"] = True
    if variant == "bias_res_bf16":
        return ops().linear(a, w, residual=res, **kw).clone()
    if variant == "res_bf16_inplace":
        x = res.clone()
        ops().linear(a, w, residual=x, out=x)
        return x
    return ops().linear(a, w, **kw).clone()


def digest(t):
    return hashlib.sha256(bits(t).cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def gelu_all_bf16():
    """Every finite bf16 value once along a row: a[:, 0] = 1, w[n, 0] = vals[n], so acc[m, n] = vals[n] exactly.  Natural order and a
    seeded column permutation; the exact result (double precision GELU, rounded to bf16) is computed once."""
    vals = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    vals = vals[torch.isfinite(vals.float())]
    assert vals.numel() == 65280
    ref = torch.nn.functional.gelu(vals.double()).float().to(torch.bfloat16)
    perm = torch.randperm(vals.numel(), generator=g(71))
    a = torch.zeros(512, 256, dtype=torch.bfloat16)
    a[:, 0] = 1.0
    return vals, ref, perm, a.to(DEV)


@pytest.mark.parametrize("order", ["natural", "permuted"])
def test_gelu_epilogue_with_values_varying_along_a_row(gelu_all_bf16, order):
    """A lane of the register-direct epilogue holds eight values of one row (columns 16 h + 4 q + r of an aligned group of 32) and
    tests them for the erfcx tail together.  With all 65 280 finite bf16 values along a row, the natural order puts the tail's
    boundary inside one block and the permutation mixes tail and non-tail values in most blocks, many with exactly one tail value:
    the tail must still be selected per element.  Both register-direct kernels equal the small-tile kernel (scalar form) bit for
    bit, every row equals row 0, and the result meets the bar of the exhaustive per-row test against the exact function."""
    vals, ref, perm, a = gelu_all_bf16
    if order == "permuted":
        vals, ref = vals[perm], ref[perm]
    n = vals.numel()
    tail = (vals.float() * 0.70710678118654752440 < -GELU_ZM).view(n // 32, 2, 4, 4)      # [group of 32][h][q][r]
    per_block = tail.sum(dim=(1, 3))                                                      # lane blocks: (group, q)
    if order == "permuted":
        assert int((per_block == 1).sum()) > 100, "the permutation leaves no lane block with exactly one tail value"
    else:
        assert int(((per_block > 0) & (per_block < 8)).sum()) >= 1
    w = torch.zeros(n, 256, dtype=torch.bfloat16)
    w[:, 0] = vals
    wd = w.to(DEV)
    outs = run_selects(lambda: ops().linear(a, wd, act="gelu"), (1, 60, 20))
    for sel in (60, 20):
        assert torch.equal(bits(outs[1]), bits(outs[sel])), f"select {sel} differs from the small-tile kernel"
    got_all = outs[60]
    assert bool((bits(got_all) == bits(got_all[:1])).all()), "rows differ"
    got = got_all[0].cpu()
    near = vals.float() >= -6.5
    same = bits(got) == bits(ref)
    miss = ~same & near
    print(f"{order}: {int(miss.sum())} inputs >= -6.5 off: {vals[miss].tolist()}")
    assert int(miss.sum()) <= 2, vals[miss].tolist()
    # the misses are one ulp off (neighbouring bit patterns); x = -0 reaches the epilogue as +0 (the accumulation drops the sign), so
    # its result differs from the exact -0 in the sign bit alone
    one_ulp = (bits(got).int() - bits(ref).int()).abs() <= 1
    assert bool((one_ulp | ((got == 0) & (ref == 0)))[miss].all())
    assert float((got.float() - ref.float())[near].abs().max()) <= 2.0 ** -7
    assert float(got[~near].float().abs().max()) <= 2.5e-10


@pytest.mark.parametrize("variant", VARIANTS)
def test_epilogue_bits_are_those_of_the_recorded_commit(variant):
    """SHA-256 of the output bytes of each epilogue variant of the flow64 test at its smallest shape (ragged M, a one-wave last
    tile column, minimum K), recorded at the commit named in the golden file, before the epilogues were rewritten."""
    M, N, K = 700, 640, 256
    golden = json.loads(GOLDEN.read_text())
    a = torch.randn(M, K, generator=g(53)).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g(54)) * 0.05).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g(55)) * 0.1).to(torch.bfloat16).to(DEV)
    res = torch.randn(M, N, generator=g(56)).to(torch.bfloat16).to(DEV)
    outs = run_selects(lambda: variant_output(variant, a, w, bias, res), (60, 20))
    for sel in (60, 20):
        d = digest(outs[sel])
        print(f"{variant} select {sel}: {d}")
        assert d == golden["sha256"][variant], f"select {sel}: output bytes differ from those of {golden['commit']}"


@pytest.mark.parametrize("variant", ["bias", "bias_res_bf16", "res_bf16_inplace"])
def test_non_finite_bias_gives_the_same_bits(variant):
    """NaN and +-Inf in a few bias columns (and so in whole output columns; Inf - Inf against the residual): the pair-wise add and
    conversion give the bits of the scalar ones."""
    M, N, K = 700, 640, 256
    a = torch.randn(M, K, generator=g(53)).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g(54)) * 0.05).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g(55)) * 0.1).to(torch.bfloat16)
    bias[[0, 5, 130, 639]] = float("nan")
    bias[[1, 6, 257, 512]] = float("inf")
    bias[[2, 7, 258, 638]] = float("-inf")
    bias = bias.to(DEV)
    res = torch.randn(M, N, generator=g(56)).to(torch.bfloat16)
    res[:, 1] = float("-inf")                       # Inf - Inf -> NaN in the residual add
    res[:, 2] = float("inf")
    res = res.to(DEV)
    if variant == "res_bf16_inplace":               # the in-place form with the bias as well
        def fn():
            x = res.clone()
            ops().linear(a, w, bias=bias, residual=x, out=x)
            return x
    else:
        fn = lambda: variant_output(variant, a, w, bias, res)
    outs = run_selects(fn, (1, 60))
    assert bool(torch.isnan(outs[1][:, 0]).all()) and bool(torch.isinf(outs[1][:, 6]).all())
    assert torch.equal(bits(outs[1]), bits(outs[60]))
