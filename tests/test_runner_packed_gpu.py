"""licv_idefics_text_forward_packed (csrc/runner.hip): the language stack of a right-padded batch on its real rows only, against the
unpacked runner (licv_idefics_text_forward, reached below the engine's length read) on the padded batch.  GEMM rows and row kernels are independent row by row and a real token never sees a padding key, so
real positions must come out BIT-IDENTICAL wherever the gate of ops.pack_rows_plan opens; padding positions are zeros when packed (and
also where the lengths were read but the rows stayed padded, so that the logits never depend on the gate)."""
import pytest
import torch

from licv.config import IDEFICS_MID
from licv.synthetic import synth_idefics_weights, synth_vqa_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = IDEFICS_MID


def _shapes():
    H, I = ARCH.hidden_size, ARCH.intermediate_size
    return [(3 * H, H), (H, H), (2 * I, H), (H, I)]


def _batch_where_the_gate_opens(B, S, parts=1, **kw):
    """The first seed whose every slice packs (decided on the CPU, as the engine does)."""
    from licv import ops
    for seed in range(2, 12):
        batch = synth_vqa_batch(ARCH, B, S, 2, seed=seed, min_len=130, dtype=torch.bfloat16, **kw)
        lens = batch["attention_mask"].sum(-1).tolist()
        cut = [B * i // parts for i in range(parts + 1)]
        if all(ops.pack_rows_plan(lens[cut[i]:cut[i + 1]], S, _shapes()) is not None for i in range(parts)):
            return {k: v.to(DEV) for k, v in batch.items()}
    raise AssertionError("no seed opens the packing gate")


class _Counted:
    def __init__(self, fn):
        self.fn, self.calls, self.any = fn, 0, 0

    def __call__(self, *a):
        self.any += 1
        self.calls += 1 if a[4] else 0                  # pack_rows: the stack runs on packed rows (0 = padded rows, padding zeroed)
        return self.fn(*a)


def _unpacked(eng, batch, parts=1, **kw):
    """Today's entry point: below IdeficsEngine.forward's length read nothing knows the lengths, so licv_idefics_text_forward runs."""
    args = (batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["image_attention_mask"], None)
    n0 = eng._runner._fn_packed.any
    out = eng._forward_slices(parts, *args, **kw) if parts > 1 else eng._forward_one(*args, **kw)
    assert eng._runner._fn_packed.any == n0
    return out


@pytest.fixture(scope="module")
def engines():
    from licv.idefics_engine import IdeficsEngine, IdeficsWeights
    from licv.runner import TextRunner
    w = IdeficsWeights(synth_idefics_weights(ARCH, seed=3, dtype=torch.float32), ARCH, DEV)
    packed, padded = IdeficsEngine(w), IdeficsEngine(w)
    packed.pack_rows, padded.pack_rows = True, False
    for e in (packed, padded):
        e._runner = TextRunner(w)
        e._runner._fn_packed = _Counted(e._runner._fn_packed)
    return packed, padded


def _hooks():
    g = torch.Generator().manual_seed(5)
    icv = (torch.randn(1, ARCH.num_layers, ARCH.hidden_size, generator=g) * 0.05).to(DEV)
    alpha = torch.full((1, ARCH.num_layers), 0.3, device=DEV)
    layers = list(range(ARCH.num_layers))
    return {"no hooks": {}, "icv": dict(icv=icv, hook_layers=layers), "icv + alpha": dict(icv=icv, alpha=alpha, hook_layers=layers),
            "subset": dict(icv=icv[:, :2].contiguous(), hook_layers=[1, 3])}


def _check(got, want, mask, what):
    real = mask.bool()
    assert got.shape == want.shape
    assert torch.equal(got[real], want[real]), f"{what}: real positions differ"
    assert bool((got[~real] == 0).all()), f"{what}: padding positions of the packed forward are not zeros"


def test_packed_runner_matches_the_padded_runner_bit_for_bit(engines):
    packed, padded = engines
    B, S = 4, 320
    batch = _batch_where_the_gate_opens(B, S)
    mask = batch["attention_mask"]
    for name, kw in _hooks().items():
        n0 = packed._runner._fn_packed.calls
        got, want = packed.forward(**batch, **kw), _unpacked(padded, batch, **kw)
        assert packed._runner._fn_packed.calls == n0 + 1, f"{name}: the packed runner was not taken"
        _check(got, want, mask, name)
        _check(padded.forward(**batch, **kw), want, mask, name + ", packing switched off")     # padded rows, padding zeroed all the same
    # logits_rows: each question's last real token and its last (padding) position
    lens = mask.sum(-1)
    base = torch.arange(B, device=DEV) * S
    rows = torch.stack([base + lens - 1, base + S - 1], 1).reshape(-1)
    kw = _hooks()["icv"]
    got, want = packed.forward(**batch, **kw, logits_rows=rows), _unpacked(padded, batch, **kw, logits_rows=rows)
    is_real = mask.reshape(-1)[rows].bool()
    assert bool((~is_real).any()) and got.shape == want.shape
    assert torch.equal(got[is_real], want[is_real]) and bool((got[~is_real] == 0).all())
    assert padded._runner._fn_packed.calls == 0


def test_left_padded_batch_takes_the_padded_path(engines):
    packed, padded = engines
    batch = {k: v.to(DEV) for k, v in synth_vqa_batch(ARCH, 4, 320, 2, seed=2, min_len=130, dtype=torch.bfloat16, padding_side="left").items()}
    n0 = packed._runner._fn_packed.any
    kw = _hooks()["icv"]
    got, want = packed.forward(**batch, **kw), _unpacked(padded, batch, **kw)
    assert packed._runner._fn_packed.any == n0
    assert torch.equal(got, want)


def test_both_slices_of_a_two_stream_batch_pack(engines):
    packed, padded = engines
    B, S = 8, 520
    batch = _batch_where_the_gate_opens(B, S, parts=2)
    assert packed.batch_streams == 2 and padded.batch_streams == 2
    n0 = packed._runner._fn_packed.calls
    kw = _hooks()["icv"]
    got, want = packed.forward(**batch, **kw), _unpacked(padded, batch, parts=2, **kw)
    assert packed._runner._fn_packed.calls == n0 + 2
    _check(got, want, batch["attention_mask"], "two slices")
