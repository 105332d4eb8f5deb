"""CPU restatement of sampled decoding (csrc/sample.hip, the SAMPLE path of csrc/beam.hip): Philox4x32-10, the kept set of
top-k / top-p / min-p with the kernels' tie rules, the inverse-CDF draw and the Gumbel-top-k draw, in numpy.  The GPU tests
(test_sample_step_gpu.py, test_beam_sample_gpu.py, test_generate_sample_gpu.py) compare the kernels against these functions
exactly; the tests here pin the restatement itself: Philox to known answers, the kept sets to transformers' own warpers, the
Gumbel draw to sequential sampling without replacement."""
import numpy as np
import pytest
import torch

MASK32 = 0xFFFFFFFF


def philox(seed, c0, c1, c2, c3):
    """Philox4x32-10 keyed by the 64-bit seed (low word first); counters broadcast as numpy arrays.  Returns the 4 output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(seed & MASK32), np.uint64((seed >> 32) & MASK32)
    m0, m1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [v.astype(np.uint32) for v in c]


def uniform(x):
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(x):
    return (-np.log(-np.log(uniform(x)))).astype(np.float32)


def okey(y):
    b = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.int64)


def mass(y, m):
    w = np.exp((y - m).astype(np.float32)).astype(np.float32)
    return w, np.floor(w.astype(np.float64) * 2.0 ** 40).astype(np.uint64)


def kept_mask(y, top_k=50, top_p=1.0, min_p=0.0, mtk=1):
    """Kept set of one row of processed scores y (float32): top-k (every score >= the k-th largest), then top-p (remove in ascending
    score order, the higher id first among equal scores, while the removed 2^-40 fixed-point mass stays <= (1 - top_p) * total),
    then min-p (exp(y - max) >= min_p); each keeps at least mtk.  Every kept set is a prefix of (score desc, id asc)."""
    y = np.asarray(y, dtype=np.float32)
    V = y.size
    key, ids = okey(y), np.arange(V)
    order = np.lexsort((ids, -key))
    m = y.max()
    w, q = mass(y, m)
    N = V
    if top_k > 0:
        k = max(int(top_k), mtk)
        if k < V:
            N = int((key >= key[order[k - 1]]).sum())
    if top_p < 1.0:
        asc = order[:N][::-1]
        cum = np.cumsum(q[asc], dtype=np.uint64)
        om = np.float32(1.0 - float(np.float32(top_p)))
        bound = np.uint64(np.floor(float(om) * float(cum[-1])))
        N = max(N - int((cum <= bound).sum()), mtk)
    if min_p > 0.0:
        N = max(int((w[order[:N]] >= np.float32(min_p)).sum()), mtk)
    keep = np.zeros(V, dtype=bool)
    keep[order[:N]] = True
    return keep, q


def sample_row(y, u, **warp):
    """Inverse CDF over the kept tokens in token-id order: the smallest id whose prefix mass exceeds floor(u * total)."""
    keep, q = kept_mask(y, mtk=1, **warp)
    ids = np.nonzero(keep)[0]
    cum = np.cumsum(q[ids], dtype=np.uint64)
    Z = int(cum[-1])
    target = min(int(np.floor(u * float(Z))), Z - 1)
    return int(ids[np.searchsorted(cum, np.uint64(target), side="right")])


def sample_step(logits, seed, step, unfinished, eos, pad, suppress_eos, temperature=1.0, **warp):
    """licv_sample_step on (B, V) fp32 logits: the token of every row (pad for finished rows) and the new unfinished flags."""
    B, V = logits.shape
    u = uniform(philox(seed, step, np.arange(B), 0, 0)[0])
    toks, unf = [], []
    for r in range(B):
        if not unfinished[r]:
            toks.append(pad); unf.append(False); continue
        x = np.asarray(logits[r], dtype=np.float32).copy()
        if suppress_eos and eos is not None and eos >= 0:
            x[eos] = -np.inf
        y = (x / np.float32(temperature)).astype(np.float32)
        t = sample_row(y, float(u[r]), **warp)
        toks.append(t); unf.append(not (eos is not None and eos >= 0 and t == eos))
    return np.array(toks, dtype=np.int64), np.array(unf)


def beam_scores(x, temperature, suppress_eos, eos):
    """Processed scores of one beam row: (log_softmax(x) with EOS suppressed) / T in fp32."""
    x = np.asarray(x, dtype=np.float32)
    mx = x.max()
    lse = np.float32(np.log(np.exp((x - mx).astype(np.float64)).sum()))
    y = (((x - mx).astype(np.float32) - lse).astype(np.float32) / np.float32(temperature)).astype(np.float32)
    if suppress_eos and eos is not None and eos >= 0:
        y[eos] = -np.inf
    return y


def gumbel_select(logits, run_scores, seed, step, temperature=1.0, suppress_eos=False, eos=None, **warp):
    """The draw of one beam-sampling step on (B, nb, V) fp32 logits and (B, nb) running scores: per question the 2*nb largest
    keys (score + running + Gumbel noise; ties: the lower flat index).  Returns (un-noised scores, flat indices, error)."""
    B, nb, V = logits.shape
    keep_n = 2 * nb
    top_lp = np.zeros((B, keep_n), dtype=np.float32)
    top_ix = np.zeros((B, keep_n), dtype=np.int64)
    err = False
    for b in range(B):
        accs, keys = [], []
        for k in range(nb):
            y = beam_scores(logits[b, k], temperature, suppress_eos, eos)
            keep, _ = kept_mask(y, mtk=2, **warp)
            acc = (y + np.float32(run_scores[b, k])).astype(np.float32)
            g = gumbel(philox(seed, step, b, k, np.arange(V))[0])
            key = np.where(keep & (acc > -np.inf), (acc + g).astype(np.float32), -np.inf).astype(np.float32)
            accs.append(np.where(keep, acc, -np.inf).astype(np.float32)); keys.append(key)
        acc, key = np.concatenate(accs), np.concatenate(keys)
        order = np.lexsort((np.arange(nb * V), -key.astype(np.float64)))[:keep_n]
        amax = acc.max()
        if not all(key[i] > -np.inf and np.exp(np.float32(acc[i] - amax)) > 0 for i in order):
            err = True
        top_lp[b], top_ix[b] = acc[order], order
    return top_lp, top_ix, err


def beam_bookkeep(st, top_lp, top_ix, eos, length_penalty=1.0, early_stopping=False):
    """The bookkeeping half of oracle.generate_ref.beam_step (its selections made stable) (transformers' _beam_search after _get_top_k_continuations) on given
    continuations, updating `st` in place.  Returns (search continues?, flat source-beam index of every new running beam)."""
    top_lp, top_ix = torch.as_tensor(top_lp), torch.as_tensor(top_ix)
    B, nb = st["run_scores"].shape
    V = st["V"]
    cur, P, max_len = st["cur"], st["P"], st["max_len"]
    keep = 2 * nb
    top_mask = torch.cat([torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool)])
    running, finished, fin_scores = st["running"], st["finished"], st["fin_scores"]
    is_fin, improve, gen_len = st["is_fin"], st["improve"], st["gen_len"]

    def gather(t, idx):
        ix = idx
        while ix.dim() < t.dim():
            ix = ix.unsqueeze(-1)
        return torch.gather(t, 1, ix.expand(*idx.shape, *t.shape[2:]))

    src = top_ix // V
    top_seq = gather(running, src)
    top_seq[:, :, cur] = top_ix % V
    hits = (top_seq[:, :, cur] == eos) | (cur + 1 >= max_len) if eos is not None else torch.full_like(top_ix, cur + 1 >= max_len, dtype=torch.bool)
    run_lp = top_lp + hits.float() * -1.0e9
    # sampled continuations tie more often than searched ones (equal bf16 logits give equal scores in any order of the draw): the
    # kernel's selections are stable - the earlier continuation first - and so are these
    nxt_ix = torch.sort(run_lp, dim=1, descending=True, stable=True)[1][:, :nb]
    running, run_scores, beam_src = gather(top_seq, nxt_ix), gather(run_lp, nxt_ix), gather(src, nxt_ix)
    just = hits & top_mask[None, :]
    fin_lp = top_lp / ((cur + 1 - P) ** length_penalty)
    fin_lp = fin_lp + (torch.all(is_fin, dim=-1, keepdim=True) & (early_stopping is True)).float() * -1.0e9
    fin_lp = fin_lp + (~improve).float() * -1.0e9 + (~just).float() * -1.0e9
    m_sc = torch.cat([fin_scores, fin_lp], 1)
    best = torch.sort(m_sc, dim=1, descending=True, stable=True)[1][:, :nb]
    finished = gather(torch.cat([finished, top_seq], 1), best)
    is_fin = gather(torch.cat([is_fin, just], 1), best)
    gen_len = gather(torch.cat([gen_len, torch.full_like(top_ix, cur + 1 - P)], 1), best)
    fin_scores = gather(m_sc, best)
    flat = (beam_src + torch.arange(B)[:, None] * nb).reshape(-1)
    cur += 1
    best_run = run_scores[:, :1] / (float(cur - P) ** length_penalty)
    worst = torch.where(is_fin, fin_scores.min(dim=1, keepdim=True)[0], torch.full_like(fin_scores, -1.0e9))
    improve = improve & torch.any(best_run > worst, dim=-1, keepdim=True)
    st.update(running=running, finished=finished, run_scores=run_scores, fin_scores=fin_scores, is_fin=is_fin, improve=improve,
              gen_len=gen_len, cur=cur)
    cont = bool(improve.any()) and not (bool(is_fin.all()) and early_stopping is True) and not bool(hits.all())
    return cont, flat


# ---------------------------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    # produced once from rocRAND's header-only rocrand_philox4x32_10.h (philox4x32_10_engine(seed, subsequence, 4 * counter_xy)
    # .next4(), a host compile): counter (x, y) = the 64-bit offset / 4, (z, w) = the subsequence.  The first row is also
    # Random123's published known answer for Philox4x32-10 at a zero key and counter.
    cases = [((0, 0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0x0123456789ABCDEF, 0, 0, 0, 0), (0xB850222E, 0xC58CB04B, 0x14A7A020, 0x7A84FFF9)),
             ((42, 3, 7, 1, 5), (0x9D514874, 0x7BB0A292, 0xD34522F0, 0xDCED2C5F))]
    for (seed, *ctr), want in cases:
        got = tuple(int(v) for v in philox(seed, *ctr))
        assert got == want, (seed, ctr, [hex(v) for v in got])


def test_uniform_and_gumbel_stay_finite():
    x = np.array([0, 255, 256, MASK32], dtype=np.uint32)
    u = uniform(x)
    assert u[0] == u[1] == 2.0 ** -25 and 0 < u.min() and u.max() < 1
    assert np.isfinite(gumbel(x)).all()


def _rows(seed, n, V):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, V)) * 2.0).astype(np.float32)          # continuous values: no boundary ties


@pytest.mark.parametrize("mtk", [1, 2])
def test_kept_sets_equal_transformers_warpers(mtk):
    tr = pytest.importorskip("transformers")
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rows = _rows(7 + mtk, 6, 1000)
    for T, k, p, mp in ((1.0, 50, 1.0, 0.0), (0.7, 0, 0.9, 0.0), (1.5, 50, 0.3, 0.0), (1.0, 0, 1.0, 0.05), (0.7, 20, 0.9, 0.05),
                        (1.0, 1, 1.0, 0.0), (1.0, 0, 0.001, 0.0)):
        for x in rows:
            if mtk == 2:                                              # the beam form: the warpers act on log_softmax
                y = torch.log_softmax(torch.from_numpy(x)[None], -1)
            else:
                y = torch.from_numpy(x)[None]
            procs = [TemperatureLogitsWarper(T)] if T != 1.0 else []
            if k:
                procs.append(TopKLogitsWarper(top_k=k, min_tokens_to_keep=mtk))
            if p < 1.0:
                procs.append(TopPLogitsWarper(top_p=p, min_tokens_to_keep=mtk))
            if mp:
                procs.append(MinPLogitsWarper(min_p=mp, min_tokens_to_keep=mtk))
            s = y / T if T != 1.0 else y
            ref = y
            for pr in procs:
                ref = pr(None, ref)
            want = torch.isfinite(ref[0]).numpy()
            got, _ = kept_mask(s[0].numpy().astype(np.float32), top_k=k, top_p=p, min_p=mp, mtk=mtk)
            assert np.array_equal(got, want), (T, k, p, mp, int(got.sum()), int(want.sum()))


def test_top_p_ties_remove_the_higher_id_first():
    y = np.array([0.0, 1.0, 1.0, 1.0, 3.0], dtype=np.float32)
    w = np.exp(y - 3.0).astype(np.float32)
    # remove the 0.0 entry and exactly one of the three equal entries: the highest id (3) goes first
    frac = (w[0] + w[1] * 1.5) / w.sum()
    keep, _ = kept_mask(y, top_k=0, top_p=float(1.0 - frac), mtk=1)
    assert keep.tolist() == [False, True, True, False, True]


def test_inverse_cdf_draw_follows_the_kept_distribution():
    y = np.log(np.array([0.5, 0.25, 0.125, 0.125], dtype=np.float32))
    xs = philox(99, 0, np.arange(4000), 0, 0)[0]
    toks = np.array([sample_row(y, float(u), top_k=0) for u in uniform(xs)])
    freq = np.bincount(toks, minlength=4) / toks.size
    assert np.abs(freq - [0.5, 0.25, 0.125, 0.125]).max() < 0.03


def test_gumbel_top_k_is_sampling_without_replacement():
    """The ordered pair of the two largest Gumbel keys has the law of two sequential draws without replacement (checked once at a
    fixed seed, 20000 trials, V = 4)."""
    p = np.array([0.4, 0.3, 0.2, 0.1])
    lp = np.log(p).astype(np.float32)
    n = 20000
    g = gumbel(philox(1234, 0, np.arange(n)[:, None], 0, np.arange(4)[None, :])[0])
    keys = lp[None, :] + g
    top2 = np.argsort(-keys, axis=1)[:, :2]
    counts = np.zeros((4, 4))
    np.add.at(counts, (top2[:, 0], top2[:, 1]), 1)
    want = np.array([[0 if i == j else p[i] * p[j] / (1 - p[i]) for j in range(4)] for i in range(4)])
    assert np.abs(counts / n - want).max() < 0.012
