"""CPU half of the CLIP text tower: the restatement (tests/clip_text_ref.py) against the transformers fixture g19, the host logic of
the packed engine (pack_text_batch, ClipTextArch.from_hf, clip_text_state), the text side of MMTopkRetriever's constructor, and the
library's new symbols."""
import types

import numpy as np
import pytest
import torch

import clip_text_ref as R


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ restatement vs transformers
@pytest.mark.parametrize("eos", [2, 95])
def test_restatement_matches_the_transformers_fixture(golden, eos):
    arch, sd, ids, mask, want = R.load_g19(golden("g19_clip_text_tiny"), eos)
    out = R.clip_text_forward(sd, arch, ids, mask, dtype=torch.float32)
    assert len(out["hidden_states"]) == arch.num_hidden_layers + 1
    for i, h in enumerate(out["hidden_states"]):
        assert _rel(R.valid_rows(h, mask), want[f"hidden_{i}"]) <= 1e-5
    assert _rel(out["text_embeds"], want["text_embeds"]) <= 1e-5
    assert _rel(out["features"], want["features"]) <= 1e-5


def test_fixture_tells_the_two_pooling_rules_apart(golden):
    g = golden("g19_clip_text_tiny")
    differ = np.abs(g["eos2::text_embeds"] - g["eos95::text_embeds"]).max(1) > 0
    assert differ.tolist() == [False] * 7 + [True]          # the unpadded row without an eos id: largest id vs position 0


def test_a_right_padded_row_and_the_same_row_alone_give_the_same_embedding(golden):
    """What makes the packed form exact: the tower is causal, padding sits to the right, so no valid token ever sees it."""
    arch, sd, ids, mask, _ = R.load_g19(golden("g19_clip_text_tiny"), 95)
    batch = R.clip_text_forward(sd, arch, ids, mask)["text_embeds"]
    for i in (0, 3, 5):
        n = int(mask[i].sum())
        alone = R.clip_text_forward(sd, arch, ids[i:i + 1, :n], mask[i:i + 1, :n])["text_embeds"]
        assert _rel(alone[0], batch[i]) <= 1e-6


# ------------------------------------------------------------------------------------------------ pack_text_batch
def test_pack_text_batch_on_the_fixture_rows(golden):
    from licv.clip_engine import pack_text_batch
    g = golden("g19_clip_text_tiny")
    lens = g["lengths"].tolist()
    for eos, last in ((2, 40), (95, 0)):
        arch, _, ids, mask, _ = R.load_g19(g, eos)
        pk = pack_text_batch(ids, mask, arch)
        cu = np.concatenate([[0], np.cumsum(lens)])
        assert pk.cu_seqlens.dtype == torch.int32 and pk.cu_seqlens.tolist() == cu.tolist()
        assert pk.ids.dtype == torch.int64 and torch.equal(pk.ids, torch.cat([ids[i, :n] for i, n in enumerate(lens)]))
        assert pk.positions.dtype == torch.int32 and pk.positions.tolist() == [p for n in lens for p in range(n)]
        # the pooled position inside each row: the last token, except the second eos id of row 4 and the row without one
        inside = [n - 1 for n in lens]
        inside[4], inside[7] = 5, last
        assert pk.pool_rows.dtype == torch.int32 and pk.pool_rows.tolist() == (cu[:-1] + np.array(inside)).tolist()
        assert torch.equal(pk.pool_rows.long() - pk.cu_seqlens[:-1].long(), R.pooled_positions(ids, eos))
        ids_, cu_, rows_ = pk[:3]                              # packed ids, cu_seqlens, pooling rows: the first three fields
        assert ids_ is pk.ids and cu_ is pk.cu_seqlens and rows_ is pk.pool_rows


def test_pack_text_batch_pooling_rules():
    from licv.clip_engine import pack_text_batch
    from licv.config import ClipTextArch
    ids = torch.tensor([[1, 7, 50, 9, 3, 0, 0], [1, 40, 8, 40, 6, 5, 4]])
    mask = torch.tensor([[1, 1, 1, 1, 1, 0, 0], [1] * 7])
    old = ClipTextArch(vocab_size=64, hidden_size=128, num_attention_heads=2, eos_token_id=2)
    assert pack_text_batch(ids, mask, old).pool_rows.tolist() == [2, 5 + 1]          # the largest id, first occurrence: not the last token
    new = ClipTextArch(vocab_size=64, hidden_size=128, num_attention_heads=2, eos_token_id=9)
    with pytest.raises(ValueError, match="row 1"):                                   # row 1's first 9 sits behind its two valid tokens
        pack_text_batch(torch.tensor([[1, 9, 0], [1, 5, 9]]), torch.tensor([[1, 1, 0], [1, 1, 0]]), new)
    assert pack_text_batch(ids, mask, new).pool_rows.tolist() == [3, 5 + 0]
    assert pack_text_batch(ids[:1], None, new).cu_seqlens.tolist() == [0, 7]         # no mask: every position is valid


def test_pack_text_batch_refuses_what_the_packed_tower_cannot_run():
    from licv.clip_engine import pack_text_batch
    from licv.config import ClipTextArch
    arch = ClipTextArch(vocab_size=96, hidden_size=128, num_attention_heads=2, max_position_embeddings=77, eos_token_id=95)
    ok = torch.tensor([[1, 5, 95, 95]])
    pack_text_batch(ok, torch.tensor([[1, 1, 1, 0]]), arch)
    with pytest.raises(ValueError, match="prefix of ones"):
        pack_text_batch(ok, torch.tensor([[1, 0, 1, 0]]), arch)                      # a hole in the mask
    with pytest.raises(ValueError, match="prefix of ones"):
        pack_text_batch(ok, torch.tensor([[0, 1, 1, 1]]), arch)                      # left padding
    with pytest.raises(ValueError, match="empty"):
        pack_text_batch(ok, torch.tensor([[0, 0, 0, 0]]), arch)
    long = torch.full((1, 78), 5)
    long[0, -1] = 95
    with pytest.raises(ValueError, match="77 positions"):
        pack_text_batch(long, torch.ones(1, 78, dtype=torch.int64), arch)
    pack_text_batch(long[:, 1:], torch.ones(1, 77, dtype=torch.int64), arch)
    with pytest.raises(ValueError, match="vocabulary"):
        pack_text_batch(torch.tensor([[1, 96, 95]]), torch.ones(1, 3, dtype=torch.int64), arch)
    with pytest.raises(ValueError, match="vocabulary"):
        pack_text_batch(torch.tensor([[1, -1, 95]]), torch.ones(1, 3, dtype=torch.int64), arch)
    with pytest.raises(ValueError, match="padding"):
        pack_text_batch(ok, torch.tensor([[1, 1, 0, 0]]), arch)                      # the first eos id sits in the padding


# ------------------------------------------------------------------------------------------------ config and state dict
B32_TEXT = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu", eos_token_id=2)


def test_clip_text_arch_from_the_three_config_shapes():
    from licv.config import CLIP_TEXT_B32, ClipTextArch
    assert CLIP_TEXT_B32.to_dict() == dict(B32_TEXT, projection_dim=512) and CLIP_TEXT_B32.head_dim == 64
    flat = dict(B32_TEXT, projection_dim=512, model_type="clip_text_model")
    assert ClipTextArch.from_hf(flat) == CLIP_TEXT_B32                                # a CLIPTextModelWithProjection config.json
    full = dict(projection_dim=512, text_config=dict(B32_TEXT, projection_dim=640), vision_config=dict(hidden_size=768))
    assert ClipTextArch.from_hf(full) == CLIP_TEXT_B32                                # a full CLIPModel config.json: the top level wins
    obj = types.SimpleNamespace(projection_dim=512, text_config=types.SimpleNamespace(**B32_TEXT))
    assert ClipTextArch.from_hf(obj) == CLIP_TEXT_B32                                 # config objects
    with pytest.raises(KeyError, match="eos_token_id"):
        ClipTextArch.from_hf({k: v for k, v in flat.items() if k != "eos_token_id"})


def test_clip_text_arch_names_the_limit_it_refuses():
    from licv.config import ClipTextArch
    with pytest.raises(ValueError, match="head_dim 32"):
        ClipTextArch.from_hf(dict(B32_TEXT, projection_dim=512, num_attention_heads=16))
    with pytest.raises(ValueError, match="max_position_embeddings 129"):
        ClipTextArch.from_hf(dict(B32_TEXT, projection_dim=512, max_position_embeddings=129))
    ClipTextArch.from_hf(dict(B32_TEXT, projection_dim=512, max_position_embeddings=128))
    with pytest.raises(ValueError, match="hidden_act"):
        ClipTextArch.from_hf(dict(B32_TEXT, projection_dim=512, hidden_act="relu"))


def test_clip_text_state_keeps_the_text_keys_only(golden):
    from licv.clip_engine import clip_text_state, clip_vision_state
    from licv.config import ClipTextArch
    from licv.synthetic import synth_clip_text_weights
    arch, sd, _, _, _ = R.load_g19(golden("g19_clip_text_tiny"), 95)
    synth = synth_clip_text_weights(arch, seed=1, dtype=torch.float32)
    assert set(synth) == set(sd) and all(synth[k].shape == sd[k].shape for k in sd)   # the generator writes the HF key names
    full = dict(sd, **{"vision_model.embeddings.class_embedding": torch.zeros(4), "visual_projection.weight": torch.zeros(4, 4),
                       "logit_scale": torch.zeros(())})
    assert set(clip_text_state(full)) == set(sd)
    with pytest.raises(KeyError, match="text tower"):
        clip_text_state({k: v for k, v in full.items() if not k.startswith("text_")})
    with pytest.raises(KeyError):
        clip_vision_state(sd)


# ------------------------------------------------------------------------------------------------ MMTopkRetriever, host side
class _StubText:
    def __init__(self, arch, sd, device):
        self.arch = arch

    def encode(self, input_ids, attention_mask):
        f = torch.nn.functional.one_hot(input_ids[:, 1] % 16, 16).float() + 0.01
        return f / f.norm(dim=-1, keepdim=True)


class _StubVision:
    def __init__(self, arch, sd, device):
        self.arch = arch

    def encode(self, pix):
        f = pix.float().reshape(pix.shape[0], -1)[:, :16]
        return f / f.norm(dim=-1, keepdim=True)


def _tok(texts, padding=True, return_tensors="pt", truncation=True):
    assert padding is True and return_tensors == "pt" and truncation is True
    ids = torch.tensor([[1, len(t), 2] for t in texts])
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def _archs(text_proj=16, vision_proj=16):
    from licv.config import ClipTextArch, ClipVisionArch
    return (ClipTextArch(vocab_size=96, hidden_size=128, num_attention_heads=2, projection_dim=text_proj),
            ClipVisionArch(hidden_size=64, num_attention_heads=4, image_size=8, patch_size=4, projection_dim=vision_proj))


def test_mapping_form_of_clip_weights_builds_only_the_towers_the_mode_needs(tmp_path, monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import licv.clip_engine
    monkeypatch.setattr(licv.clip_engine, "ClipTextEngine", _StubText)
    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", lambda *a, **k: pytest.fail("image tower built for mode 't2t'"))
    tarch, varch = _archs()
    texts = [dict(text="x" * n) for n in range(1, 10)]
    r = M.MMTopkRetriever(texts, texts[2:4], "some/clip", "t2t", "text", "text", 4, 0, str(tmp_path / "t.pkl"), "cpu",
                          clip_weights={"text": (tarch, {}), "tokenizer": _tok})
    assert r.index_features.shape == (9, 16) and r.test_features.shape == (2, 16) and r.index_features.dtype == np.float32
    assert np.array_equal(r.test_features, r.index_features[2:4])
    assert torch.load(tmp_path / "t.pkl", weights_only=False)["meta_info"]["mode"] == "t2t"
    # mixed mode: both towers, the test side (first letter) through the image tower
    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", _StubVision)
    images = [dict(image=torch.randn(3, 8, 8)) for _ in range(3)]
    r = M.MMTopkRetriever(texts, images, "some/clip", batch_size=4, cache_file=None, device="cpu",
                          clip_weights={"vision": (varch, {}), "text": (tarch, {}), "tokenizer": _tok}, img_processor=torch.stack)
    assert r.mode == "i2t" and r.index_features.shape == (9, 16) and r.test_features.shape == (3, 16)
    # the 2-tuple keeps its meaning: the image tower
    r = M.MMTopkRetriever(images, images, "some/clip", "i2i", "image", "image", 4, 0, None, "cpu", clip_weights=(varch, {}),
                          img_processor=torch.stack)
    assert r.index_features.shape == (3, 16)


def test_projection_mismatch_in_a_mixed_mode_is_refused_before_any_tower_is_built(monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import licv.clip_engine
    monkeypatch.setattr(licv.clip_engine, "ClipTextEngine", lambda *a, **k: pytest.fail("tower built"))
    monkeypatch.setattr(licv.clip_engine, "ClipVisionEngine", lambda *a, **k: pytest.fail("tower built"))
    tarch, varch = _archs(text_proj=16, vision_proj=32)
    with pytest.raises(ValueError, match="32 and 16"):
        M.MMTopkRetriever([dict(text="a")], [dict(image=None)], "some/clip", "i2t",
                          clip_weights={"vision": (varch, {}), "text": (tarch, {}), "tokenizer": _tok})


def test_default_tokenizer_is_one_local_autotokenizer_call(tmp_path, monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import licv.clip_engine
    import transformers
    calls = []

    def from_pretrained(name, **kw):
        calls.append((name, kw))
        return _tok

    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(from_pretrained))
    monkeypatch.setattr(licv.clip_engine, "ClipTextEngine", _StubText)
    monkeypatch.setenv("MODEL_CPK_DIR", str(tmp_path))
    (tmp_path / "clip-vit-base-patch32").mkdir()
    tarch, _ = _archs()
    texts = [dict(text="x" * n) for n in range(1, 6)]
    M.MMTopkRetriever(texts, texts, mode="t2t", test_field="text", batch_size=8, device="cpu", clip_weights={"text": (tarch, {})})
    assert calls == [(str(tmp_path / "clip-vit-base-patch32"), {"local_files_only": True})]
    # the tower, too, comes from that directory when none is given
    loaded = []
    monkeypatch.setattr(licv.clip_engine, "load_clip_text", lambda p: loaded.append(p) or (tarch, {}))
    M.MMTopkRetriever(texts, texts, mode="t2t", test_field="text", batch_size=8, device="cpu")
    assert loaded == [tmp_path / "clip-vit-base-patch32"] and len(calls) == 2


def test_text_mode_without_a_tower_says_no_local_checkpoint_was_found(monkeypatch):
    from icv_src.utils import mm_topk_retriver as M
    import transformers
    monkeypatch.delenv("MODEL_CPK_DIR", raising=False)
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: pytest.fail("tokenizer work before the raise")))
    _, varch = _archs()
    for weights in (None, (varch, {}), {"vision": (varch, {}), "tokenizer": _tok}):
        with pytest.raises(NotImplementedError, match="'t2i'.*no local checkpoint was found"):
            M.MMTopkRetriever([dict(image=None)], [dict(text="a")], mode="t2i", index_field="image", test_field="text", clip_weights=weights)


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_are_declared_and_exported_and_the_version_stays_9():
    from licv import _lib
    new = {"licv_clip_text_embed", "licv_attn_varlen_causal", "licv_layernorm_rows_fwd"}
    assert new <= set(_lib.declared_symbols())
    assert _lib.header_abi_version() == 9 and _lib.ABI_VERSION == 9
    l = _lib.lib()
    assert all(hasattr(l, s) for s in new) and l.licv_version() == 9
    assert _lib.check_exports()


def test_attn_varlen_causal_checks_its_arguments_on_the_host_before_any_launch():
    """The refusals read the host copy of cu_seqlens only and launch nothing, so they can be seen without a GPU (the device pointers
    are never dereferenced on these paths)."""
    import ctypes as C
    from licv import _lib
    l = _lib.lib()
    fake = C.c_void_p(4096)

    def status(cu, n_heads=2, head_dim=64, ld=384):
        a = np.asarray(cu, dtype=np.int32)
        return l.licv_attn_varlen_causal(fake, ld, C.c_void_p(a.ctypes.data), fake, len(cu) - 1, n_heads, head_dim, C.c_float(0.125), fake, None)

    for kw, word in ((dict(cu=[0, 5], head_dim=32), b"head_dim"), (dict(cu=[0, 0, 5]), b"length 0"), (dict(cu=[0, 129]), b"length 129"),
                     (dict(cu=[0, 5, 3]), b"length -2"), (dict(cu=[1, 5]), b"must be 0"), (dict(cu=[0, 5], ld=383), b"ld_qkv"),
                     (dict(cu=[0, 5], ld=376), b"ld_qkv")):
        assert status(**kw) == -1 and word in l.licv_last_error(), (kw, l.licv_last_error())
