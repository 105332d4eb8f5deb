"""Seeded data sets and the validity checker of the exact inner-product search (licv_topk_ip): shared by tests/test_retriever_cpu.py
(which checks the checker) and tests/test_topk_ip_gpu.py (which applies it to the kernel).  An ordinary helper module."""
from __future__ import annotations

import numpy as np

# (Q, N, D, k) of the GPU test
SHAPES = [(1, 64, 32, 1), (7, 1000, 512, 32), (256, 20000, 512, 32), (64, 100000, 512, 16), (33, 4097, 768, 64), (5, 64, 1024, 64)]
# planted cosines: 0.95, 0.945, ... (0.635 at k = 64); the step is 80 x tau at D = 1024
PLANT_TOP, PLANT_STEP = 0.95, 0.005


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def planted(Q, N, D, k, seed):
    """-> (queries (Q, D) fp32, index (N, D) fp32, expected (P, k) int64): for the first P queries the k best rows are constructed at
    cosines 0.95, 0.945, ... and scattered to random positions; every other row stays below 0.5 against EVERY query by construction
    (queries are mutually orthogonal; planted rows have no component along the other queries; filler rows have their query components
    replaced by a combination of norm 0.3).  P = as many queries as fit into half of N."""
    assert Q < D
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.standard_normal((D, Q)))            # (D, Q), orthonormal columns
    queries = basis.T.copy()

    def off_queries(n):                                             # unit rows orthogonal to every query
        u = rng.standard_normal((n, D))
        u -= (u @ basis) @ basis.T
        return _unit(u)

    filler = off_queries(N)
    mix = _unit(rng.standard_normal((N, Q))) * 0.3                  # cosines against the queries: at most 0.3
    index = mix @ basis.T + np.sqrt(1 - 0.09) * filler
    P = min(Q, (N // 2) // k)
    expected = np.zeros((P, k), dtype=np.int64)
    if P:
        spots = rng.permutation(N)[:P * k].reshape(P, k)
        cos = PLANT_TOP - PLANT_STEP * np.arange(k)
        for p in range(P):
            index[spots[p]] = cos[:, None] * queries[p][None, :] + np.sqrt(1 - cos ** 2)[:, None] * off_queries(k)
            expected[p] = spots[p]
    return queries.astype(np.float32), index.astype(np.float32), expected


# Width of the clustered cloud.  0.7 everywhere but at (33, 4097, 768, 64): 64 of 4097 neighbours at tau(768) sit so close at 0.7 that only
# 38 % of the (row, rank) positions are isolated by 2 tau in float64 (measured on the float64 list alone); 1.5 gives 60 %.
CLUSTER_NOISE = {(33, 4097, 768, 64): 1.5}


def clustered(Q, N, D, seed, noise=0.7):
    """Unit rows around a common mean (mean + noise x a vector of unit expected norm): all cosines high, neighbours close, like CLIP
    features."""
    rng = np.random.default_rng(seed)
    mean = _unit(rng.standard_normal(D))
    mk = lambda n: _unit(mean[None, :] + noise * rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
    return mk(Q), mk(N)


def with_ties(q, x, seed, queries=(0,)):
    """For each listed query: its best match (float64) is copied, bit for bit, to two more scattered positions.  -> (index, {query: the
    three positions, ascending})."""
    rng = np.random.default_rng(seed)
    x = x.copy()
    taken, out = set(), {}
    for qi in queries:
        s = q[qi].astype(np.float64) @ x.astype(np.float64).T
        best = int(np.argmax(s))
        spots = [best]
        while len(spots) < 3:
            c = int(rng.integers(0, x.shape[0]))
            if c not in spots and c not in taken:
                spots.append(c)
        x[spots[1]] = x[best]
        x[spots[2]] = x[best]
        taken.update(spots)
        out[qi] = sorted(spots)
    return x, out


def scores64(q, x):
    return q.astype(np.float64) @ x.astype(np.float64).T


def tau_matrix(q, x):
    """First-order bound on an fp32 dot product in any summation order: D * 2^-24 * |q| * |x| (3.05e-5 for D = 512 unit rows)."""
    D = q.shape[1]
    return D * 2.0 ** -24 * np.linalg.norm(q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(x.astype(np.float64), axis=1)[None, :]


def check_topk(q, x, k, idx, score):
    """Validity of a (Q, k) search result against float64 scores s and tau (tau_matrix).  Raises AssertionError naming the first
    clause that fails; returns the share of (row, rank) positions that fell under the exact clause.
      1 indices in range and distinct per row;
      2 |score[j] - s[idx[j]]| <= tau;
      3 s[idx[j]] >= s[idx[j+1]] - 2 tau;
      4 every index left out has s <= s[idx[k-1]] + 2 tau;
      5 a rank whose float64 score is more than 2 tau away from both neighbours in the float64 order (rank k counts as a neighbour)
        holds exactly the float64 list's index."""
    idx, score = np.asarray(idx), np.asarray(score)
    Q, N = q.shape[0], x.shape[0]
    assert idx.shape == (Q, k) and score.shape == (Q, k), (idx.shape, score.shape)
    assert idx.dtype == np.int64 and score.dtype == np.float32
    assert ((idx >= 0) & (idx < N)).all(), "clause 1: index out of range"
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "clause 1: repeated index in a row"
    s, T = scores64(q, x), tau_matrix(q, x)
    rows = np.arange(Q)[:, None]
    s_out, t_out = s[rows, idx], T[rows, idx]
    err = np.abs(score.astype(np.float64) - s_out)
    assert (err <= t_out).all(), f"clause 2: returned score off by {err.max():.3e} (tau {t_out.max():.3e})"
    if k > 1:
        gap = s_out[:, :-1] - s_out[:, 1:] + (t_out[:, :-1] + t_out[:, 1:])
        assert (gap >= 0).all(), f"clause 3: row not sorted, worst inversion {-gap.min():.3e} beyond 2 tau"
    left = np.ones((Q, N), dtype=bool)
    left[rows, idx] = False
    over = np.where(left, s - (s_out[:, -1:] + T + t_out[:, -1:]), -np.inf)
    assert (over <= 0).all(), f"clause 4: an index left out beats the last one returned by {over.max():.3e} beyond 2 tau"
    kk = min(k + 1, N)
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    s_ref, t_ref = s[rows, order], T[rows, order]
    d = s_ref[:, :-1] - s_ref[:, 1:]                                 # gap between ranks j and j+1
    wide = d > (t_ref[:, :-1] + t_ref[:, 1:])
    iso = np.ones((Q, k), dtype=bool)
    iso[:, 1:] &= wide[:, :k - 1]
    if kk > k:
        iso &= wide[:, :k]
    else:                                                            # N == k: the last rank has no lower neighbour
        iso[:, :k - 1] &= wide[:, :k - 1]
    bad = iso & (idx != order[:, :k])
    assert not bad.any(), f"clause 5: {int(bad.sum())} isolated ranks hold another index than the float64 list"
    return float(iso.mean())


def ties_in_order(idx, score):
    """The tie rule of licv_topk_ip: wherever two neighbouring ranks of a row return bit-equal scores, the lower index comes first."""
    idx, bits = np.asarray(idx), np.asarray(score).view(np.uint32)
    same = bits[:, 1:] == bits[:, :-1]
    return bool((~same | (idx[:, :-1] < idx[:, 1:])).all())


def topk_numpy_fp32(q, x, k):
    """numpy's own fp32 product + stable argsort (score descending, index ascending)."""
    s = q @ x.T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return order.astype(np.int64), np.take_along_axis(s, order, axis=1)
