"""CPU half of RICE retrieval: the validity checker the GPU test relies on (accepts the float64 reference and numpy's fp32 product,
rejects a swapped neighbour, bf16-rounded inputs and a tie resolved upwards) on every data set the GPU test uses, and the host logic
of MMTopkRetriever (cache-file layout in both directions, no device when loading from a cache, text modes, reversed order, errors)."""
import numpy as np
import pytest
import torch

import retrieval_data as RD
from clip_ref import topk_ip_ref


def _bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def _datasets():
    for shape in RD.SHAPES:
        Q, N, D, k = shape
        q, x, _ = RD.planted(Q, N, D, k, seed=11)
        yield ("planted", shape, q, x)
        q, x = RD.clustered(Q, N, D, seed=12, noise=RD.CLUSTER_NOISE.get(shape, 0.7))
        yield ("clustered", shape, q, x)


@pytest.mark.parametrize("kind,shape,q,x", list(_datasets()), ids=lambda v: v if isinstance(v, str) else ("x".join(map(str, v)) if isinstance(v, tuple) else ""))
def test_checker_accepts_the_references_and_rejects_wrong_results(kind, shape, q, x):
    Q, N, D, k = shape
    idx, score = topk_ip_ref(q, x, k)
    share = RD.check_topk(q, x, k, idx, score)
    if kind == "clustered":
        assert share >= 0.5, f"generator condition: only {share:.3f} of the positions are isolated by 2 tau"
    i32, s32 = RD.topk_numpy_fp32(q, x, k)
    RD.check_topk(q, x, k, i32, s32)
    if kind == "planted" and k > 1:
        P = min(Q, (N // 2) // k)
        if P:
            assert (idx[:P] == RD.planted(Q, N, D, k, seed=11)[2]).all()
    s = RD.scores64(q, x)
    # (a) one neighbour swapped for a clearly worse one (the worst row of the index for query 0)
    bad_i, bad_s = idx.copy(), score.copy()
    worst = int(np.argmin(s[0]))
    if worst not in idx[0]:
        bad_i[0, k // 2] = worst
        bad_s[0, k // 2] = np.float32(s[0, worst])
        with pytest.raises(AssertionError, match="clause"):
            RD.check_topk(q, x, k, bad_i, bad_s)
    # (b) scores from bf16-rounded inputs
    if D >= 512:
        ib, sb = RD.topk_numpy_fp32(_bf16_round(q), _bf16_round(x), k)
        with pytest.raises(AssertionError, match="clause"):
            RD.check_topk(q, x, k, ib, sb)


def test_checker_rejects_a_tie_resolved_to_the_higher_index():
    Q, N, D, k = 7, 1000, 512, 32
    q, x = RD.clustered(Q, N, D, seed=14)
    x, triples = RD.with_ties(q, x, seed=15, queries=(0, Q - 1))
    idx, score = topk_ip_ref(q, x, k)
    RD.check_topk(q, x, k, idx, score)
    for qi, spots in triples.items():
        assert idx[qi, :3].tolist() == spots
    assert RD.ties_in_order(idx, score)
    flipped = idx.copy()
    flipped[0, [0, 1]] = flipped[0, [1, 0]]
    RD.check_topk(q, x, k, flipped, score)                      # the tau clauses cannot see it ...
    assert not RD.ties_in_order(flipped, score)                 # ... the tie rule does


# ------------------------------------------------------------------------------------------------ MMTopkRetriever, host side
def _unit_rows(n, d, seed):
    a = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _reference_style_cache(path, index, test, mode="i2i"):
    torch.save({"index_features": index, "test_features": test,
                "meta_info": {"clip_model_name": "openai/clip-vit-base-patch32", "mode": mode, "index_field": "image", "test_field": "image"}}, path)


def test_loading_from_a_cache_file_never_touches_the_device_or_builds_a_tower(tmp_path, monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import licv.clip_engine
    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", lambda *a, **k: pytest.fail("tower built although a cache file exists"))
    index, test = _unit_rows(50, 32, 1), _unit_rows(4, 32, 2)
    f = tmp_path / "rice.pkl"
    _reference_style_cache(f, index, test)
    for mode in ("i2i", "i2t", "t2i", "t2t"):                    # text modes work from a cache
        r = M.MMTopkRetriever([], [], mode=mode, index_field="image", cache_file=str(f), device="cuda")
        assert r.index_features.dtype == np.float32 and np.array_equal(r.index_features, index) and np.array_equal(r.test_features, test)
        assert r._index_dev is None
    assert not torch.cuda.is_initialized() or torch.cuda.is_available()


def test_text_modes_raise_when_features_have_to_be_computed(tmp_path):
    from icv_src.utils.mm_topk_retriver import MMTopkRetriever
    for mode in ("i2t", "t2i", "t2t"):
        with pytest.raises(NotImplementedError, match=mode):
            MMTopkRetriever([{"image": None, "text": "a"}], [{"image": None, "text": "b"}], mode=mode, cache_file=str(tmp_path / "none.pkl"))
    with pytest.raises(NotImplementedError, match="i2t"):       # the class default mode, as in the reference
        MMTopkRetriever([{"image": None}], [{"image": None}])


def test_unresolvable_model_name_names_the_places_tried(tmp_path, monkeypatch):
    from icv_src.utils.mm_topk_retriver import MMTopkRetriever, resolve_clip_dir
    monkeypatch.setenv("MODEL_CPK_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        MMTopkRetriever([{"image": None}], [{"image": None}], mode="i2i", index_field="image")
    msg = str(e.value)
    assert "openai/clip-vit-base-patch32" in msg and str(tmp_path / "openai/clip-vit-base-patch32") in msg and "no network" in msg
    (tmp_path / "clip-vit-base-patch32").mkdir()
    assert resolve_clip_dir("openai/clip-vit-base-patch32") == tmp_path / "clip-vit-base-patch32"
    monkeypatch.delenv("MODEL_CPK_DIR")
    with pytest.raises(FileNotFoundError, match="MODEL_CPK_DIR is not set"):
        resolve_clip_dir("openai/clip-vit-base-patch32")


def test_constructor_surface_matches_the_reference():
    import inspect
    from icv_src.utils.mm_topk_retriver import MMTopkRetriever
    sig = inspect.signature(MMTopkRetriever.__init__)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD][1:]
    assert pos == [("index_ds", inspect._empty), ("test_ds", inspect._empty), ("clip_model_name", "openai/clip-vit-base-patch32"),
                   ("mode", "i2t"), ("index_field", "text"), ("test_field", "image"), ("batch_size", 1), ("num_workers", 0),
                   ("cache_file", None), ("device", "cuda"), ("reversed_order", False)]
    assert [n for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY] == ["clip_weights", "img_processor"]


def test_retrieve_goes_through_one_search_and_reverses_on_request(tmp_path, monkeypatch):
    """The search itself is a GPU kernel (tests/test_topk_ip_gpu.py); here it is replaced by the float64 reference to check the
    plumbing around it: one call over all test rows, lists of ints, reversed_order."""
    from icv_src.utils import mm_topk_retriver as M
    from licv import ops
    index, test = _unit_rows(50, 32, 1), _unit_rows(4, 32, 2)
    f = tmp_path / "rice.pkl"
    _reference_style_cache(f, index, test)
    calls = []

    def fake_topk(q, x, k):
        calls.append((tuple(q.shape), tuple(x.shape), k))
        i, s = topk_ip_ref(q.numpy(), x.numpy(), k)
        return torch.from_numpy(i), torch.from_numpy(s)

    monkeypatch.setattr(ops, "topk_ip", fake_topk)
    want = topk_ip_ref(test, index, 5)[0].tolist()
    r = M.MMTopkRetriever([], [], mode="i2i", index_field="image", cache_file=str(f), device="cpu")
    assert r.retrieve(5) == want and calls == [((4, 32), (50, 32), 5)]
    assert all(isinstance(v, int) for row in r.retrieve(2) for v in row)
    rev = M.MMTopkRetriever([], [], mode="i2i", index_field="image", cache_file=str(f), device="cpu", reversed_order=True)
    assert rev.retrieve(5) == [list(reversed(w)) for w in want]


def test_cache_written_here_has_the_references_layout(tmp_path, monkeypatch):
    """create_index with the tower replaced by a stub: the file holds what the reference's torch.save call holds, and loads back."""
    from icv_src.utils import mm_topk_retriver as M
    import licv.clip_engine

    class StubTower:
        arch = type("A", (), {"image_size": 8})()

        def __init__(self, arch, sd, device):
            pass

        def encode(self, pix):
            f = pix.float().reshape(pix.shape[0], -1)[:, :16]
            return f / f.norm(dim=-1, keepdim=True)

    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", StubTower)
    g = torch.Generator().manual_seed(3)
    proc = lambda images: torch.stack(images)
    train = [{"image": torch.randn(3, 8, 8, generator=g), "question": f"q{i}"} for i in range(9)]
    val = [{"image": train[i]["image"] + 0.01, "question": "?"} for i in (4, 2)]
    f = tmp_path / "cache" / "rice.pkl"
    f.parent.mkdir()
    r = M.MMTopkRetriever(train, val, "some/clip", "i2i", "image", "image", 4, 2, str(f), "cpu", clip_weights=(None, {}), img_processor=proc)
    saved = torch.load(f, weights_only=False)
    assert set(saved) == {"index_features", "test_features", "meta_info"}
    assert saved["meta_info"] == {"clip_model_name": "some/clip", "mode": "i2i", "index_field": "image", "test_field": "image"}
    assert isinstance(saved["index_features"], np.ndarray) and saved["index_features"].dtype == np.float32 and saved["index_features"].shape == (9, 16)
    assert saved["test_features"].shape == (2, 16) and np.array_equal(saved["index_features"], r.index_features)
    assert np.abs(np.linalg.norm(r.index_features.astype(np.float64), axis=1) - 1).max() < 1e-6
    again = M.MMTopkRetriever(train, val, "some/clip", "i2i", "image", "image", cache_file=str(f), device="cpu")
    assert np.array_equal(again.test_features, r.test_features)
    # cache_file=None computes and does not save (the reference fails in torch.save(..., None))
    M.MMTopkRetriever(train, val, "some/clip", "i2i", "image", "image", 4, 0, None, "cpu", clip_weights=(None, {}), img_processor=proc)
