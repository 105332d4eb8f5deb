"""licv_logits_process (csrc/logits_process.hip) against the plain-torch restatement of transformers' processors
(tests/logits_process_ref.py, held equal to the transformers classes by tests/test_logits_process_ref_cpu.py).

normalize = 0: every output is the fp32 input, one fp32 product or quotient of it, or -inf -> torch.equal.
normalize = 1: the log-softmax is a reduction whose order differs from torch's, so the un-processed output is held to the project's
bar for fp32 beam scores, 2e-5 * (1 + max|ref|) of a float64 log-softmax (tests/test_beam_step_gpu.py), and the processed output is
bit-equal to the restatement applied to the kernel's OWN un-processed output (the processors are again one IEEE operation each)."""
import ctypes as C

import pytest
import torch

from logits_process_ref import process

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 2
N = 3                                     # n-gram size of the mixed cases: histories of n - 2, n - 1 and n tokens are below
CURS = sorted({1, N - 2, N - 1, N, 37, 830})


def _case(V, cur, P, seed, R=6):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, min(V, 24), (R, 840), generator=g)           # few distinct tokens: duplicates and repeated n-grams
    ids[:, ::5] = torch.randint(0, V, (R, 168), generator=g)            # ... and some from the whole vocabulary (the last word of the maps)
    ids[0, :] = V - 1
    h = ids[1, :cur].tolist()
    words = [[7], [EOS], [V - 1, 5], h[-2:] + [11], [(h[-1] + 1) % V, 12], h + [14], list(range(min(cur + 3, V)))]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=N, bad_words_ids=words, suppress_tokens=[0, 3, V - 2],
              begin_suppress_tokens=[1, 4, V - 3])
    return ids, kw


def _gpu(logits, ids, cur, P, kw, **opt):
    from licv.ops import LogitsConstraints, logits_process
    cons = LogitsConstraints(DEV, eos=EOS, **kw)
    return logits_process(logits, ids.to(DEV), cur, P, cons, **opt).cpu()     # (ids rows are longer than cur: ids_ld > cur)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [96, 100, 32002])
def test_logits_process_matches_the_restatement(V, dtype):
    R, ld = 6, V + 11
    g = torch.Generator().manual_seed(V)
    buf = (torch.randn(R, ld, generator=g) * 4.0).to(dtype)
    logits = buf.to(DEV)[:, :V]                                          # a view with ld > V, as the LM head returns it
    x32 = buf[:, :V].float()
    plain = _gpu(logits, torch.zeros((R, 1), dtype=torch.long), 1, 1, {})
    assert torch.equal(plain, x32)                                       # nothing on: the fp32 value of the logit
    lp0 = _gpu(logits, torch.zeros((R, 1), dtype=torch.long), 1, 1, {}, normalize=True)
    ref64 = torch.log_softmax(buf[:, :V].double(), -1)
    assert float((lp0.double() - ref64).abs().max()) <= 2e-5 * (1 + float(ref64.abs().max()))
    for cur in CURS:
        for P in sorted({cur, max(1, cur - 3)}):                         # the first generated token (begin list on) and later ones
            ids, kw = _case(V, cur, P, 1000 * cur + P)
            ref = process(x32, ids[:, :cur], P, eos=EOS, **kw)
            got = _gpu(logits, ids, cur, P, kw)
            assert torch.equal(got, ref) and torch.equal(torch.isinf(got), torch.isinf(ref)), (cur, P)
            assert int(torch.isinf(ref).sum()) > 0
            for one in ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "begin_suppress_tokens"):   # each alone
                k1 = {one: kw[one]}
                assert torch.equal(_gpu(logits, ids, cur, P, k1), process(x32, ids[:, :cur], P, eos=EOS, **k1)), (cur, P, one)
            got = _gpu(logits, ids, cur, P, kw, normalize=True)
            ref = process(lp0, ids[:, :cur], P, eos=EOS, **kw)
            assert torch.equal(got, ref) and torch.equal(torch.isinf(got), torch.isinf(ref)), (cur, P, "normalize")


@pytest.mark.parametrize("n", [1, 2, 4])
def test_ngram_sizes_and_penalties_below_one(n):
    V, R, cur = 100, 6, 37
    g = torch.Generator().manual_seed(n)
    x = torch.randn(R, V, generator=g) * 4.0
    ids = torch.randint(0, 6, (R, cur), generator=g)
    kw = dict(no_repeat_ngram_size=n, repetition_penalty=0.8)
    assert torch.equal(_gpu(x.to(DEV), ids, cur, 30, kw), process(x, ids, 30, **kw))


@pytest.mark.parametrize("V", [32768, 32769, 65536])
def test_vocabularies_around_the_wide_variant(V):
    """Up to 32768 entries a lane holds 32 of them, above 64 (another instantiation); 65536 is the limit."""
    R, cur, P = 6, 37, 37
    x = (torch.randn(R, V, generator=torch.Generator().manual_seed(V)) * 4.0).to(torch.bfloat16)
    ids, kw = _case(V, cur, P, V)
    got = _gpu(x.to(DEV), ids, cur, P, kw)
    assert torch.equal(got, process(x.float(), ids[:, :cur], P, eos=EOS, **kw))
    lp0 = _gpu(x.to(DEV), ids, cur, P, {}, normalize=True)
    ref64 = torch.log_softmax(x.double(), -1)
    assert float((lp0.double() - ref64).abs().max()) <= 2e-5 * (1 + float(ref64.abs().max()))
    assert torch.equal(_gpu(x.to(DEV), ids, cur, P, kw, normalize=True), process(lp0, ids[:, :cur], P, eos=EOS, **kw))


def test_shared_rows_serve_all_beams_of_a_question():
    V, B, nb, cur = 100, 3, 2, 37
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, V + 4, generator=g) * 4.0).to(torch.bfloat16)
    ids, kw = _case(V, cur, cur, 77, R=B * nb)
    for normalize in (False, True):
        got = _gpu(x.to(DEV)[:, :V], ids, cur, cur, kw, nb=nb, shared_rows=True, normalize=normalize)
        dense = _gpu(x[:, :V].repeat_interleave(nb, 0).contiguous().to(DEV), ids, cur, cur, kw, nb=nb, normalize=normalize)
        assert torch.equal(got, dense)
    assert torch.equal(got[:, :V].isinf(), process(x[:, :V].float().repeat_interleave(nb, 0), ids[:, :cur], cur, eos=EOS, **kw).isinf())


def test_logits_process_rejects_bad_arguments():
    from licv import _lib
    lib = _lib.lib()
    t = torch.zeros(64, device=DEV)

    def args(**over):
        a = _lib.LogitsProcessArgs()
        a.logits, a.logits_dtype, a.ld, a.q_stride_rows, a.beam_stride_rows = t.data_ptr(), _lib.LICV_F32, 8, 1, 1
        a.B, a.nb, a.V, a.ids, a.ids_ld, a.cur, a.P = 1, 1, 8, t.data_ptr(), 4, 2, 1
        a.out, a.out_ld, a.repetition_penalty = t.data_ptr() + 128, 8, 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def rejected(a, text):
        return lib.licv_logits_process(C.byref(a), None) == -1 and text in lib.licv_last_error()

    assert lib.licv_logits_process(None, None) == -1
    assert rejected(args(logits=None), b"null pointer") and rejected(args(ids=None), b"null pointer") and rejected(args(out=None), b"null pointer")
    assert rejected(args(V=65537, ld=65537, out_ld=65537), b"vocabulary")
    assert rejected(args(repetition_penalty=0.0), b"repetition_penalty") and rejected(args(repetition_penalty=-1.0), b"repetition_penalty")
    assert rejected(args(cur=0, P=1), b"position")
    assert rejected(args(no_repeat_ngram_size=-1), b"no_repeat_ngram_size")
    assert rejected(args(n_bad_words=2, bad_words_len=2), b"no pointer")
    lists = dict(bad_words=t.data_ptr(), bad_offsets=t.data_ptr(), n_bad_words=2, bad_words_len=2)
    assert rejected(args(bad_offsets_host=C.cast((C.c_int32 * 3)(0, 2, 2), C.c_void_p), **lists), b"out of order")
    assert rejected(args(bad_offsets_host=C.cast((C.c_int32 * 3)(0, 1, 3), C.c_void_p), **lists), b"offsets")
    assert rejected(args(bad_offsets_host=C.cast((C.c_int32 * 3)(1, 2, 2), C.c_void_p), **lists), b"offsets")
