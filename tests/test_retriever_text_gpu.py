"""The text modes of MMTopkRetriever end to end on the GPU: "t2t" over toy texts with the tiny text tower of fixture g19 (tokenizer
callable -> packed tower -> licv_topk_ip -> cache file), and the mixed modes "i2t" / "t2i" with g18's image tower, whose projection has
the same width."""
import numpy as np
import pytest
import torch

import clip_ref as RV
import clip_text_ref as R
import retrieval_data as RD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOS, EOS = 1, 95
N_INDEX, SOURCES = 40, [3, 17, 8, 0, 21, 39, 5, 9]
TEXT_SEED, EDIT_SEED = 41, 51          # picked on the CPU so that the generator's condition below holds (margin 16 x the bf16 noise)


def toy_tokenizer(texts, padding=True, return_tensors="pt", truncation=True):
    """Whitespace words "w<id>" -> ids, bos / eos added, truncated to 77, right-padded with the eos id (as the public CLIP tokenizer pads)."""
    assert padding is True and return_tensors == "pt" and truncation is True
    rows = [[BOS] + [int(w[1:]) for w in t.split()][:75] + [EOS] for t in texts]
    S = max(map(len, rows))
    ids = torch.full((len(rows), S), EOS, dtype=torch.int64)
    mask = torch.zeros((len(rows), S), dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
        mask[i, :len(r)] = 1
    return {"input_ids": ids, "attention_mask": mask}


def toy_texts():
    rng = np.random.default_rng(TEXT_SEED)
    index = [" ".join(f"w{int(t)}" for t in rng.integers(3, 94, int(rng.integers(4, 13)))) for _ in range(N_INDEX)]
    rng = np.random.default_rng(EDIT_SEED)
    tests = []
    for s in SOURCES:                                        # one-token edits of the chosen sources
        w = index[s].split()
        w[int(rng.integers(0, len(w)))] = f"w{int(rng.integers(3, 94))}"
        tests.append(" ".join(w))
    return index, tests


def test_t2t_end_to_end(tmp_path, golden, monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    arch, sd, _, _, _ = R.load_g19(golden("g19_clip_text_tiny"), EOS)
    index, tests = toy_texts()
    train_ds = [dict(question=t, answer=f"a{i}") for i, t in enumerate(index)]
    val_ds = [dict(question=t, question_id=j) for j, t in enumerate(tests)]

    # the generator's own condition, from the CPU restatement: the source ranks first with a margin above the bf16 noise
    cos = {}
    for dt in (torch.float32, torch.bfloat16):
        f = [R.clip_text_forward(sd, arch, **toy_tokenizer(t), dtype=dt)["features"].double() for t in (tests, index)]
        cos[dt] = f[0] @ f[1].T
    c = cos[torch.float32]
    rows = torch.arange(len(SOURCES))
    own = c[rows, SOURCES]
    other = c.clone()
    other[rows, SOURCES] = -2
    margin, noise = float((own - other.max(1).values).min()), float((cos[torch.bfloat16] - c).abs().max())
    print(f"restatement: smallest margin of the source over the best other text {margin:.3e}; its own bf16 run moves a cosine by at most {noise:.3e}")
    assert margin >= 3 * noise, "generator: the edited texts are not separated from the other index texts by 3 x the bf16 noise"

    seen = []

    def tok(texts, **kw):
        seen.append(len(texts))
        return toy_tokenizer(texts, **kw)

    cache = tmp_path / "rice_textemb.pkl"
    weights = {"text": (arch, sd), "tokenizer": tok}
    r = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, clip_model_name="toy/clip", mode="t2t", index_field="question",
                          test_field="question", batch_size=16, cache_file=str(cache), device=DEV, clip_weights=weights)
    assert seen == [16, 16, 8, 8]                                                  # batch_size texts per tokenizer call, index side first
    assert r.index_features.shape == (N_INDEX, arch.projection_dim) and r.test_features.shape == (len(SOURCES), arch.projection_dim)
    assert r.index_features.dtype == np.float32 and np.abs(np.linalg.norm(r.index_features.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    assert not hasattr(r, "text_encoder") and not hasattr(r, "vision_encoder")
    got_cos = torch.from_numpy(r.test_features).double() @ torch.from_numpy(r.index_features).double().T
    print(f"engine features: cosines within {float((got_cos - c).abs().max()):.3e} of the fp32 restatement")
    top1, top4 = r.retrieve(1), r.retrieve(4)
    assert top1 == [[s] for s in SOURCES]
    assert [row[0] for row in top4] == SOURCES and all(len(set(row)) == 4 for row in top4)

    saved = torch.load(cache, weights_only=False)
    assert set(saved) == {"index_features", "test_features", "meta_info"}
    assert saved["meta_info"] == {"clip_model_name": "toy/clip", "mode": "t2t", "index_field": "question", "test_field": "question"}
    assert isinstance(saved["index_features"], np.ndarray) and np.array_equal(saved["index_features"], r.index_features)
    assert np.array_equal(saved["test_features"], r.test_features)

    # a second instance from the cache file: same lists, no tower, no tokenizer
    import licv.clip_engine
    monkeypatch.setattr(licv.clip_engine, "ClipTextEngine", lambda *a, **k: pytest.fail("tower built although the cache file exists"))
    again = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, mode="t2t", index_field="question", test_field="question",
                              cache_file=str(cache), device=DEV)
    assert again.retrieve(4) == top4 and again.retrieve(1) == top1
    rev = M.MMTopkRetriever(index_ds=train_ds, test_ds=val_ds, mode="t2t", index_field="question", test_field="question",
                            cache_file=str(cache), device=DEV, reversed_order=True)
    assert rev.retrieve(4) == [list(reversed(row)) for row in top4]


@pytest.mark.parametrize("mode", ["i2t", "t2i"])
def test_mixed_modes(golden, mode):
    from icv_src.utils import mm_topk_retriver as M
    from licv import ops
    tarch, tsd, _, _, _ = R.load_g19(golden("g19_clip_text_tiny"), EOS)
    varch, vsd, pix = RV.load_g18(golden("g18_clip_tiny"))
    assert tarch.projection_dim == varch.projection_dim
    index_texts, test_texts = toy_texts()
    images = [dict(image=p) for p in pix]
    weights = {"vision": (varch, vsd), "text": (tarch, tsd), "tokenizer": toy_tokenizer}
    if mode == "i2t":                                      # test side images, index side texts (the class defaults' fields)
        index_ds, test_ds, fields = [dict(text=t) for t in index_texts], images, dict(index_field="text", test_field="image")
    else:
        index_ds, test_ds, fields = images, [dict(text=t) for t in test_texts], dict(index_field="image", test_field="text")
    r = M.MMTopkRetriever(index_ds, test_ds, "toy/clip", mode, batch_size=16, device=DEV, clip_weights=weights,
                          img_processor=lambda ims: torch.stack(ims), **fields)
    D = tarch.projection_dim
    assert r.index_features.shape == (len(index_ds), D) and r.test_features.shape == (len(test_ds), D)
    for f in (r.index_features, r.test_features):
        assert f.dtype == np.float32 and np.abs(np.linalg.norm(f.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    k = min(4, len(index_ds))
    lists = r.retrieve(k)
    idx, score = ops.topk_ip(r._test_dev, r._index_dev, k)
    assert lists == idx.tolist() and all(len(set(row)) == k and all(0 <= i < len(index_ds) for i in row) for row in lists)
    RD.check_topk(r.test_features, r.index_features, k, idx.cpu().numpy(), score.cpu().numpy())
