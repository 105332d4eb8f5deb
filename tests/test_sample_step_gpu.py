"""licv_sample_step (csrc/sample.hip) against the CPU restatement (test_sampling_ref_cpu.py), exactly: ids, pads, unfinished
flags and the continue flag, step after step, over batch sizes, vocabulary sizes, bf16 / fp32 logits with a padded row stride and
the warper settings; top_k = 1 against argmax; seeds; a chi-square check of the draw; argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_sampling_ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(B, V, dtype, T, k, p, mp, seed, steps=3, eos=2, pad=0, min_new=2, peaked=False):
    from licv.generation import SampleState, sample_params
    g = torch.Generator().manual_seed(seed)
    P = 3
    ids = torch.randint(3, V, (B, P), generator=g)
    st = SampleState(B, P, P + steps, ids.to(DEV), eos, pad, min_new, sample_params(T, k, p, mp, seed))
    unf = np.ones(B, dtype=bool)
    for s in range(steps):
        ld = (V + 7) // 8 * 8 + 8
        buf = (torch.randn(B, ld, generator=g) * (4.0 if peaked else 2.0)).to(dtype)
        if s == 2:
            buf[: B // 2, eos] = 30.0                                # some rows finish
        logits = buf.to(DEV)[:, :V]
        more = st.step(logits)
        want, unf_next = R.sample_step(buf[:, :V].float().numpy(), seed, s, unf, eos, pad, s < min_new, T, top_k=k, top_p=p, min_p=mp)
        got = st.seq[:, P + s].cpu().numpy()
        assert np.array_equal(got, want), f"step {s}: rows {np.nonzero(got != want)[0].tolist()}"
        assert np.array_equal(st.unfinished.cpu().numpy().astype(bool), unf_next)
        assert np.array_equal(st.next_tokens.cpu().numpy(), want)
        unf = unf_next
        assert more == (bool(unf.any()) and s + 1 < steps)
    return st.seq.cpu()


GRID = [(B, V, dt) for B in (1, 8) for V in (257, 32002, 32003) for dt in (torch.bfloat16, torch.float32)] + [(24, 257, torch.bfloat16)]
WARP = [(1.0, 50, 1.0, 0.0), (0.7, 0, 0.9, 0.0), (1.5, 1, 1.0, 0.05), (1.0, 0, 0.3, 0.05), (0.7, -1, 0.9, 0.0), (1.5, 50, 0.3, 0.0)]


@pytest.mark.parametrize("B,V,dtype", GRID)
def test_sample_step_equals_restatement(B, V, dtype):
    for i, (T, k, p, mp) in enumerate(WARP):
        _run(B, V, dtype, T, V if k < 0 else k, p, mp, seed=1000 * B + V + i)


def test_top_k_one_is_argmax():
    from licv.generation import SampleState, sample_params
    g = torch.Generator().manual_seed(5)
    B, V = 8, 32002
    x = torch.randn(B, V, generator=g)                               # fp32: no tie at the top
    st = SampleState(B, 1, 2, torch.zeros(B, 1, dtype=torch.long, device=DEV), None, 0, 0, sample_params(0.7, 1, 0.9, None, 3))
    st.step(x.to(DEV))
    assert torch.equal(st.seq[:, 1].cpu(), x.argmax(-1))


def test_same_seed_same_ids_other_seed_differs():
    a = _run(8, 32002, torch.bfloat16, 1.0, 0, 1.0, 0.0, seed=11, min_new=3)
    b = _run(8, 32002, torch.bfloat16, 1.0, 0, 1.0, 0.0, seed=11, min_new=3)
    assert torch.equal(a, b)
    from licv.generation import SampleState, sample_params
    x = torch.randn(8, 32002, generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = []
    for seed in (11, 12):
        st = SampleState(8, 1, 2, torch.zeros(8, 1, dtype=torch.long, device=DEV), None, 0, 0, sample_params(1.0, 0, 1.0, None, seed))
        st.step(x)
        outs.append(st.seq[:, 1].cpu())
    assert not torch.equal(outs[0], outs[1])


def test_chi_square_on_a_peaked_row():
    """One row, four tokens carry the mass; 4096 rows of the same logits are drawn at one fixed seed (every row its own counter)."""
    from licv.generation import SampleState, sample_params
    V, n = 257, 4096
    p = np.array([0.4, 0.3, 0.2, 0.1])
    x = torch.full((V,), -40.0)
    x[[5, 17, 100, 256]] = torch.log(torch.tensor(p, dtype=torch.float32))
    st = SampleState(n, 1, 2, torch.zeros(n, 1, dtype=torch.long, device=DEV), None, 0, 0, sample_params(1.0, 0, 1.0, None, 77))
    st.step(x[None].expand(n, V).contiguous().to(DEV))
    toks = st.seq[:, 1].cpu().numpy()
    counts = np.array([(toks == t).sum() for t in (5, 17, 100, 256)])
    assert counts.sum() == n
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    assert chi2 < 16.27                                              # 3 degrees of freedom, p = 0.001


def test_bad_arguments_return_badarg():
    from licv import _lib
    from licv.generation import sample_params
    L = _lib.lib()
    B, V = 2, 300
    logits = torch.zeros(B, V, device=DEV)
    ids = torch.zeros(B, 4, dtype=torch.long, device=DEV)
    unf = torch.ones(B, dtype=torch.uint8, device=DEV)
    nxt = torch.zeros(B, dtype=torch.long, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    sync = torch.zeros(2, dtype=torch.int32, device=DEV)

    def args(**over):
        a = _lib.SampleStepArgs()
        a.logits, a.logits_dtype, a.ld, a.B, a.V = logits.data_ptr(), 1, V, B, V
        a.ids, a.ids_ld, a.max_len, a.cur, a.P = ids.data_ptr(), 4, 4, 1, 1
        a.unfinished, a.next_tokens, a.eos, a.pad, a.suppress_eos = unf.data_ptr(), nxt.data_ptr(), -1, 0, 0
        a.flags, a.sync = flags.data_ptr(), sync.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    torch.cuda.synchronize()
    for a, p in ((args(), sample_params(0.0, 50, 1.0, None, 1)), (args(), sample_params(-1.0, 50, 1.0, None, 1)),
                 (args(), sample_params(1.0, 50, 0.0, None, 1)), (args(), sample_params(1.0, 50, 1.5, None, 1)),
                 (args(), sample_params(1.0, -1, 1.0, None, 1)), (args(V=65537, ld=65537), sample_params(1.0, 50, 1.0, None, 1)),
                 (args(logits=None), sample_params(1.0, 50, 1.0, None, 1)), (args(ids=None), sample_params(1.0, 50, 1.0, None, 1)),
                 (args(flags=None), sample_params(1.0, 50, 1.0, None, 1))):
        assert L.licv_sample_step(C.byref(a), C.byref(p), None) == -1
    assert L.licv_sample_step(C.byref(args()), None, None) == -1
    assert L.licv_sample_step(None, C.byref(sample_params(1.0, 50, 1.0, None, 1)), None) == -1
    assert L.licv_sample_step(C.byref(args()), C.byref(sample_params(1.0, 50, 1.0, None, 1)), None) == 0
    torch.cuda.synchronize()
    assert int(sync.sum()) == 0
