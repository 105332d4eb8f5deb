"""The engines' outputs, bit for bit, as recorded before the shared model code moved into licv/blocks.py: SHA-256 over the raw bits of
every logit tensor, token-id tensor and gradient of the cases below, and for four forwards the sequence of profiled launches (every
GEMM with its (M, N, K), every hook launch), which is the "same kernels, same order" check.  The cases use public entry points only, so
tools/make_engine_digests.py writes tests/golden/engine_digests.json from these same functions on any commit."""
import hashlib
import json
from dataclasses import replace
from functools import lru_cache
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = Path(__file__).resolve().parent / "golden" / "engine_digests.json"


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def g(seed):
    return torch.Generator().manual_seed(seed)


def profiled(fn):
    """fn() under a launch profiler (which selects the Python layer loop): its result and the (kind, label) of every launch, in order."""
    from licv import ops
    prof = []
    ops.set_profiler(prof)
    try:
        out = fn()
    finally:
        ops.set_profiler(None)
    return out, [[e[0], list(e[4]) if len(e) > 4 else None] for e in prof]


def hooks(arch):
    from licv.synthetic import synth_icv
    icv, alpha = synth_icv(arch.num_layers, arch.hidden_size, seed=31, alpha=0.1, device=DEV)
    return dict(icv=icv, alpha=alpha, hook_layers=list(range(arch.num_layers)))


# ------------------------------------------------------------------------------------------------ Idefics
@lru_cache(maxsize=None)
def idefics(preset):
    from licv.config import IDEFICS_MID, IDEFICS_TINY
    from licv.idefics_engine import IdeficsEngine, IdeficsWeights
    from licv.synthetic import synth_idefics_weights, synth_vqa_batch
    arch = {"tiny": IDEFICS_TINY, "mid": IDEFICS_MID}[preset]
    eng = IdeficsEngine(IdeficsWeights(synth_idefics_weights(arch, seed=11, dtype=torch.float32), arch, DEV))
    S = 24 if preset == "tiny" else 300                      # mid: M = 600 >= 512 rows, the folded residual adds and inject_renorm(pre=...)
    batch = synth_vqa_batch(arch, 2, S, 2, seed=12, min_len=S - 4, dtype=torch.bfloat16, device=DEV)
    return arch, eng, batch


def idefics_forward(preset):
    arch, eng, batch = idefics(preset)
    out = {}
    for name, runner in (("runner", True), ("loop", False)):
        eng.use_runner = runner
        try:
            out[f"logits_{name}"] = eng.forward(**batch, **hooks(arch))
        finally:
            eng.use_runner = True
    return out


def case_idefics_tiny():
    arch, eng, batch = idefics("tiny")
    out = idefics_forward("tiny")
    cap = {}
    out["logits_capture"] = eng.forward(**batch, **hooks(arch), capture=cap)
    out["final_norm"] = cap["final_norm"]
    for key in ("raw", "edited"):
        assert len(cap[key]) == arch.num_layers
        for i, t in enumerate(cap[key]):
            out[f"{key}_{i}"] = t
    rows = torch.tensor([3, 4, 17, 24 + 5, 24 + 19], device=DEV)
    for name, runner in (("runner", True), ("loop", False)):
        eng.use_runner = runner
        try:
            out[f"logits_rows_{name}"] = eng.forward(**batch, **hooks(arch), logits_rows=rows)
        finally:
            eng.use_runner = True
    out["encode_images"] = eng.encode_images(batch["pixel_values"])
    return out


def case_idefics_mid():
    return idefics_forward("mid")


def launches_idefics(preset):
    arch, eng, batch = idefics(preset)
    return profiled(lambda: eng.forward(**batch, **hooks(arch)))[1]


# ------------------------------------------------------------------------------------------------ Idefics2
@lru_cache(maxsize=None)
def idefics2(preset, fp8=False):
    from licv.config import IDEFICS2_MID, IDEFICS2_TINY
    from licv.idefics2_engine import Idefics2Engine, Idefics2Weights
    from licv.synthetic import synth_idefics2_weights, synth_vqa_batch_idefics2
    arch = {"tiny": IDEFICS2_TINY, "mid": IDEFICS2_MID}[preset]
    sd = synth_idefics2_weights(arch, seed=13, dtype=torch.float32)
    eng = Idefics2Engine(Idefics2Weights(sd, arch, DEV, fp8_text=fp8, fp8_vision=fp8))
    if preset == "tiny":     # ragged images under a pixel_attention_mask (attention mode 2), one all-zero padding image (dropped)
        batch = synth_vqa_batch_idefics2(arch, 2, 24, 2, 56, 56, seed=14, min_len=20, dtype=torch.bfloat16, device=DEV, ragged=True,
                                         drop_last_image_of_row0=True)
        assert not bool(batch["pixel_attention_mask"].all())
    else:                    # plain: full images, M = 600 rows
        batch = synth_vqa_batch_idefics2(arch, 2, 300, 2, 84, 84, seed=14, min_len=296, dtype=torch.bfloat16, device=DEV, ragged=False)
    return arch, eng, batch


def case_idefics2_tiny():
    arch, eng, batch = idefics2("tiny")
    cap = {}
    out = {"logits": eng.forward(**batch, **hooks(arch)), "logits_capture": eng.forward(**batch, **hooks(arch), capture=cap)}
    out["image_hidden_states"] = cap["image_hidden_states"]
    for key in ("mlp_raw", "layer_out"):
        assert len(cap[key]) == arch.num_layers
        for i, t in enumerate(cap[key]):
            out[f"{key}_{i}"] = t
    out["logits_plain"] = eng.forward(**batch)
    return out


def case_idefics2_mid():
    arch, eng, batch = idefics2("mid")
    return {"logits": eng.forward(**batch, **hooks(arch)), "logits_plain": eng.forward(**batch)}


def case_idefics2_mid_fp8():
    """fp8_text and fp8_vision: qkv_w, o_w and gu_w (K = 256) take e4m3 operands, down_w (K = 352) stays bf16; the tower's 72 rows are
    below the row threshold and stay bf16 as well."""
    arch, eng, batch = idefics2("mid", True)
    assert all(set(L.q8) == {"qkv_w", "o_w", "gu_w"} for L in eng.w.text)
    return {"logits": eng.forward(**batch, **hooks(arch)), "logits_plain": eng.forward(**batch)}


def launches_idefics2(preset, fp8=False):
    arch, eng, batch = idefics2(preset, fp8)
    return profiled(lambda: eng.forward(**batch, **hooks(arch)))[1]


# ------------------------------------------------------------------------------------------------ generate
GEN = dict(max_new_tokens=3, min_new_tokens=3, length_penalty=0.0)          # min_new_tokens: prefill and two decode steps, whatever is drawn


def case_generate_idefics():
    from licv.generation import generate
    arch, eng, batch = idefics("tiny")
    h = hooks(arch)
    icv = h["alpha"].unsqueeze(-1) * h["icv"]
    out = {}
    for name, runner in (("runner", True), ("loop", False)):
        eng.use_runner = runner
        try:
            for nb in (3, 1):
                out[f"ids_beams{nb}_{name}"] = generate(eng, **batch, icv=icv, hook_layers=h["hook_layers"], num_beams=nb, **GEN)
        finally:
            eng.use_runner = True
    return out


def case_generate_idefics2():
    from licv.generation import generate_idefics2
    arch, eng, batch = idefics2("tiny")
    h = hooks(arch)
    icv = h["alpha"].unsqueeze(-1) * h["icv"]
    return {f"ids_beams{nb}": generate_idefics2(eng, **batch, icv=icv, hook_layers=h["hook_layers"], num_beams=nb, **GEN) for nb in (3, 1)}


# ------------------------------------------------------------------------------------------------ CLIP towers
def case_clip_vision():
    from licv.clip_engine import ClipVisionEngine
    from licv.config import ClipVisionArch
    from licv.synthetic import synth_clip_vision_weights
    tiny = ClipVisionArch(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, image_size=28, patch_size=14,
                          projection_dim=32)
    pix = torch.randn(3, 3, 28, 28, generator=g(16)).to(torch.bfloat16).to(DEV)
    out = {}
    for act in ("quick_gelu", "gelu"):
        arch = replace(tiny, hidden_act=act)
        eng = ClipVisionEngine(arch, synth_clip_vision_weights(arch, seed=15), DEV)
        hs = []
        out[f"{act}_image_embeds"] = eng.image_embeds(pix, hidden_states=hs)
        assert len(hs) == arch.num_hidden_layers + 1
        for i, t in enumerate(hs):
            out[f"{act}_hidden_{i}"] = t
    return out


def case_clip_text():
    from licv.clip_engine import ClipTextEngine
    from licv.config import ClipTextArch
    from licv.synthetic import synth_clip_text_weights
    tiny = ClipTextArch(vocab_size=96, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                        max_position_embeddings=16, projection_dim=32, eos_token_id=95)
    lens = [12, 5, 9]                                                       # unequal lengths, right-padded, eos at the end of each row
    ids = torch.randint(1, 95, (3, 12), generator=g(18))
    mask = torch.zeros(3, 12, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, n - 1] = 95
        ids[r, n:] = 0
        mask[r, :n] = 1
    out = {}
    for act in ("quick_gelu", "gelu"):
        arch = replace(tiny, hidden_act=act)
        eng = ClipTextEngine(arch, synth_clip_text_weights(arch, seed=17), DEV)
        hs = []
        out[f"{act}_text_embeds"] = eng.text_embeds(ids, mask, hidden_states=hs)
        assert len(hs) == arch.num_hidden_layers + 1
        for i, t in enumerate(hs):
            out[f"{act}_hidden_{i}"] = t
    return out


# ------------------------------------------------------------------------------------------------ student passes
def student(sp, arch, batch, V):
    h = hooks(arch)
    rows = torch.tensor([5, 6, 7, 24 + 10, 24 + 11], device=DEV)
    logits, st = sp.forward(**batch, icv=h["icv"], hook_layers=h["hook_layers"], alpha=h["alpha"], logits_rows=rows)
    ld = (V + 7) // 8 * 8
    d = torch.zeros(rows.numel(), ld)
    d[:, :V] = torch.randn(rows.numel(), V, generator=g(19)) * 0.01
    grad_v = sp.backward(st, d.to(torch.bfloat16).to(DEV))
    return {"logits": logits, "grad_v": grad_v}


def case_student_idefics():
    from licv.train_engine import StudentPass, TrainWeights
    arch, eng, batch = idefics("tiny")
    return student(StudentPass(eng, TrainWeights(eng.w)), arch, batch, eng.w.lm_head.shape[0])


def case_student_idefics2():
    from licv.train_engine import StudentPass2, TrainWeights2
    arch, eng, batch = idefics2("tiny")
    return student(StudentPass2(eng, TrainWeights2(eng.w)), arch, batch, eng.w.lm_head.shape[0])


CASES = {
    "idefics_tiny": case_idefics_tiny, "idefics_mid": case_idefics_mid,
    "idefics2_tiny": case_idefics2_tiny, "idefics2_mid": case_idefics2_mid, "idefics2_mid_fp8": case_idefics2_mid_fp8,
    "generate_idefics": case_generate_idefics, "generate_idefics2": case_generate_idefics2,
    "clip_vision": case_clip_vision, "clip_text": case_clip_text,
    "student_idefics": case_student_idefics, "student_idefics2": case_student_idefics2,
}
LAUNCHES = {
    "idefics_tiny": lambda: launches_idefics("tiny"), "idefics_mid": lambda: launches_idefics("mid"),
    "idefics2_tiny": lambda: launches_idefics2("tiny"), "idefics2_mid": lambda: launches_idefics2("mid"),
    "idefics2_mid_fp8": lambda: launches_idefics2("mid", True),
}


def run_case(name):
    with torch.no_grad():
        return {k: digest(t) for k, t in CASES[name]().items()}


@pytest.mark.parametrize("name", list(CASES))
def test_output_bits_are_those_of_the_recorded_commit(name):
    golden = json.loads(GOLDEN.read_text())
    got = run_case(name)
    want = golden["sha256"][name]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    for k in got:
        print(f"{name} {k}: {got[k]}")
    assert not bad, f"{name}: {bad} differ from the bits of {golden['commit']}"


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_launch_sequence_is_that_of_the_recorded_commit(name):
    """Every GEMM's (M, N, K) and every hook launch of the Python layer loop, in order."""
    golden = json.loads(GOLDEN.read_text())
    with torch.no_grad():
        got = LAUNCHES[name]()
    want = golden["launches"][name]
    assert len(got) > 0
    assert got == want, f"{name}: launch {next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))} differs"
