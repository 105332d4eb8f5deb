"""licv_topk_ip on the GPU: planted neighbours come back exactly, clustered data passes the validity checker (tests/retrieval_data.py),
ties resolve to the lowest index, and a pair's score does not depend on where its row sits or how the call is tiled."""
import numpy as np
import pytest
import torch

import retrieval_data as RD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ops():
    from licv import ops as o
    return o


def search(q, x, k, **kw):
    idx, score = ops().topk_ip(torch.from_numpy(q).to(DEV), torch.from_numpy(x).to(DEV), k, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("shape", RD.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_planted_neighbours_come_back_exactly(shape):
    Q, N, D, k = shape
    q, x, expected = RD.planted(Q, N, D, k, seed=11)
    idx, score = search(q, x, k)
    P = expected.shape[0]
    print(f"planted {shape}: {P} of {Q} queries planted")
    assert (idx[:P] == expected).all(), f"{int((idx[:P] != expected).sum())} planted positions differ"
    share = RD.check_topk(q, x, k, idx, score)                       # every row, the unplanted ones included
    print(f"planted {shape}: exact-clause share {share:.3f}")


@pytest.mark.parametrize("shape", RD.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clustered_data_passes_the_validity_checker(shape):
    Q, N, D, k = shape
    q, x = RD.clustered(Q, N, D, seed=12, noise=RD.CLUSTER_NOISE.get(shape, 0.7))
    idx, score = search(q, x, k)
    share = RD.check_topk(q, x, k, idx, score)
    print(f"clustered {shape}: exact-clause share {share:.3f}")
    assert share >= 0.5, f"generator condition: only {share:.3f} of the positions are isolated by 2 tau"


def test_strided_rows():
    Q, N, D, k = 7, 1000, 512, 32
    q, x = RD.clustered(Q, N, D, seed=13)
    qb = torch.full((Q, D + 8), float("nan"), device=DEV)
    xb = torch.full((N, D + 12), float("nan"), device=DEV)
    qb[:, :D] = torch.from_numpy(q).to(DEV)
    xb[:, :D] = torch.from_numpy(x).to(DEV)
    idx, score = ops().topk_ip(qb[:, :D], xb[:, :D], k)
    dense = search(q, x, k)
    assert (idx.cpu().numpy() == dense[0]).all() and (score.cpu().numpy().view(np.uint32) == dense[1].view(np.uint32)).all()
    RD.check_topk(q, x, k, idx.cpu().numpy(), score.cpu().numpy())


@pytest.mark.parametrize("shape", [(7, 1000, 512, 32), (64, 100000, 512, 16), (33, 4097, 768, 64)], ids=lambda s: "x".join(map(str, s)))
def test_ties_resolve_to_the_lowest_index(shape):
    Q, N, D, k = shape
    q, x = RD.clustered(Q, N, D, seed=14)
    x, triples = RD.with_ties(q, x, seed=15, queries=(0, Q - 1))
    idx, score = search(q, x, k)
    for qi, spots in triples.items():
        assert idx[qi, :3].tolist() == spots, (qi, idx[qi, :3].tolist(), spots)
        assert len(set(score[qi, :3].view(np.uint32).tolist())) == 1
    assert RD.ties_in_order(idx, score)
    RD.check_topk(q, x, k, idx, score)


def _pairs(idx, score, rows=None):
    out = {}
    for qi in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            r = int(idx[qi, j]) if rows is None else int(rows[idx[qi, j]])
            out[(qi, r)] = int(score[qi, j:j + 1].view(np.uint32)[0])
    return out


def test_a_pairs_score_does_not_depend_on_position_or_tiling():
    Q, N, D, k = 40, 1536, 512, 64
    q, x = RD.clustered(Q, N, D, seed=16)
    rng = np.random.default_rng(17)
    base = search(q, x, k)
    again = search(q, x, k)
    assert base[0].tobytes() == again[0].tobytes() and base[1].tobytes() == again[1].tobytes()
    ref = _pairs(*base)
    perm = rng.permutation(N)
    p = _pairs(*search(q, np.ascontiguousarray(x[perm]), k), rows=perm)
    sub = np.sort(rng.permutation(N)[:N // 3])
    s = _pairs(*search(q, np.ascontiguousarray(x[sub]), k), rows=sub)
    a, b = search(q[:13], x, k), search(q[13:], x, k)
    assert np.concatenate([a[0], b[0]]).tobytes() == base[0].tobytes() and np.concatenate([a[1], b[1]]).tobytes() == base[1].tobytes()
    for name, other, least in (("permuted", p, 0.9), ("subset", s, 0.2)):
        common = ref.keys() & other.keys()
        print(f"position independence, {name}: {len(common)} pairs in both results")
        assert len(common) >= least * len(ref)
        assert all(ref[key] == other[key] for key in common), f"{name}: a pair's fp32 score changed with the row's position"
