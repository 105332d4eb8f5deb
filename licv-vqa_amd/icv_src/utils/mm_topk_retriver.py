"""Retrieval of in-context examples by CLIP similarity behind the reference's interface: `MMTopkRetriever` of
ref:icv_src/utils/mm_topk_retriver.py (the reference's spelling of the file name), as ref:inference.py:185-199 constructs it and
:204 calls it.  Same constructor surface, attributes and cache-file layout; underneath, both CLIP towers run on the native engines
(licv/clip_engine.py: the image tower, and the text tower on packed tokens) and the exact inner-product search that the reference hands
to faiss.IndexFlatIP is one fused HIP kernel (licv_topk_ip).  Equal scores resolve to the lowest index (faiss leaves ties unspecified).
All four modes compute: "i2i", "t2t", and the mixed "i2t" / "t2i" (test side first, as the reference reads the mode string).

What differs, on purpose: there is no network, so `clip_model_name` has to resolve to a local directory unless the towers are handed
over in `clip_weights`; the tokenizer is not ours - it is the one `transformers.AutoTokenizer.from_pretrained(<that directory>,
local_files_only=True)` gives, or any callable given in `clip_weights`; only the towers a mode needs are built; a text mode without a
text tower (none given, no local checkpoint) raises NotImplementedError before anything else happens; `cache_file=None` computes
without saving."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from collections.abc import Mapping
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)               # hf:utils/constants.py OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_WORKERS = 16


def resize_center_crop_u8(img, size: int) -> np.ndarray:
    """hf CLIPImageProcessor up to its rescale step, on the host with PIL: RGB, shortest edge -> size (bicubic; the long edge is
    int(size * long / short)), centre crop size x size.  -> (size, size, 3) uint8."""
    from PIL import Image
    from licv.frontend import clip_resize_geometry
    if not isinstance(img, Image.Image):
        img = Image.fromarray(np.asarray(img))
    img = img.convert("RGB")
    w, h = img.size
    (nw, nh), (left, top) = clip_resize_geometry(w, h, size)
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), resample=Image.BICUBIC)
    return np.asarray(img.crop((left, top, left + size, top + size)), dtype=np.uint8)


def _to_pil(img):
    from PIL import Image
    return Image.fromarray(np.asarray(img))


def resolve_clip_dir(name: str) -> Path:
    """`name` as given, or under $MODEL_CPK_DIR (the reference's variable for model directories): the first that is a directory."""
    tried = [Path(name)]
    root = os.environ.get("MODEL_CPK_DIR")
    if root:
        tried += [Path(root) / name, Path(root) / Path(name).name]
    for p in tried:
        if p.is_dir():
            return p
    raise FileNotFoundError(f"CLIP model {name!r} is not a local directory (config.json + *.safetensors; there is no network to fetch it). "
                            f"Tried: {', '.join(str(p) for p in tried)}" + ("" if root else " (MODEL_CPK_DIR is not set)"))


class MMTopkRetriever:
    device_resize = False      # True: resize + crop + normalise on the device (licv_resize_images, the bytes PIL would give) instead of
                               # the PIL thread pool + licv_preprocess_images; only where no img_processor is given

    def __init__(self, index_ds: Sequence[dict], test_ds: Sequence[dict], clip_model_name: Optional[str] = "openai/clip-vit-base-patch32",
                 mode: Optional[str] = "i2t", index_field: Optional[str] = "text", test_field: Optional[str] = "image",
                 batch_size: Optional[int] = 1, num_workers: Optional[int] = 0, cache_file: Optional[str] = None, device: str = "cuda",
                 reversed_order: Optional[bool] = False, *, clip_weights=None, img_processor: Optional[Callable] = None) -> None:
        """As the reference class.  Keyword-only extras: `clip_weights` = (ClipVisionArch, state dict) of an image tower held in memory,
        or a mapping with any of "vision": (ClipVisionArch, state dict), "text": (ClipTextArch, state dict), "tokenizer": a callable used as
        tok(texts, padding=True, return_tensors="pt", truncation=True) -> input_ids / attention_mask (what is not given comes from the
        local directory clip_model_name resolves to); `img_processor` = callable, list of images -> (n, 3, S, S) tensor, replacing
        the built-in CLIPImageProcessor restatement."""
        self.index_ds, self.test_ds = index_ds, test_ds
        self.clip_model_name = clip_model_name
        self.device = device
        self.batch_size = max(1, int(batch_size or 1))
        self.num_workers = max(0, min(int(num_workers or 0), MAX_WORKERS))
        self.mode = mode
        self.index_field, self.test_field = index_field, test_field
        self.reversed_order = reversed_order
        self._clip_weights, self._img_processor = clip_weights, img_processor
        self._index_dev = self._test_dev = None
        if cache_file is None or not os.path.exists(cache_file):
            self.create_index(cache_file)
        else:
            features = torch.load(cache_file, weights_only=False)       # the reference's layout: numpy arrays in a pickled dict
            self.index_features = np.ascontiguousarray(features["index_features"], dtype=np.float32)
            self.test_features = np.ascontiguousarray(features["test_features"], dtype=np.float32)

    # ------------------------------------------------------------------------------------------ features
    def _given(self, what: str):
        """The entry `what` ("vision", "text", "tokenizer") of clip_weights, or None; the 2-tuple form is the image tower."""
        cw = self._clip_weights
        if isinstance(cw, Mapping):
            return cw.get(what)
        return cw if what == "vision" else None

    def create_index(self, cache_file: Optional[str]) -> None:
        index_enc, test_enc = self.mode.split("2")[1], self.mode.split("2")[0]
        need = {index_enc, test_enc}
        clip_dir = None
        if "t" in need and self._given("text") is None:
            try:
                clip_dir = resolve_clip_dir(self.clip_model_name)
            except (FileNotFoundError, TypeError) as e:
                raise NotImplementedError(f"mode {self.mode!r} needs the CLIP text tower: none was given in clip_weights and no local checkpoint "
                                          f"was found for {self.clip_model_name!r} ({e}); compute 'i2i' features, pass the tower, or pass a "
                                          f"cache_file written by the reference") from None
        from licv import clip_engine as CE
        local = lambda: clip_dir if clip_dir is not None else resolve_clip_dir(self.clip_model_name)
        towers = {}
        if "i" in need:
            towers["i"] = self._given("vision") or CE.load_clip_vision(local())
        if "t" in need:
            towers["t"] = self._given("text") or CE.load_clip_text(local())
        if len(towers) == 2 and towers["i"][0].projection_dim != towers["t"][0].projection_dim:
            raise ValueError(f"mode {self.mode!r} compares image and text features, but the towers project to {towers['i'][0].projection_dim} "
                             f"and {towers['t'][0].projection_dim} dimensions")
        if "t" in need:
            self.tokenizer = self._given("tokenizer")
            if self.tokenizer is None:
                from transformers import AutoTokenizer
                self.tokenizer = AutoTokenizer.from_pretrained(str(local()), local_files_only=True)
            self.text_encoder = CE.ClipTextEngine(*towers["t"], self.device)
        if "i" in need:
            self.vision_encoder = CE.ClipVisionEngine(*towers["i"], self.device)
        encode = {"i": self.encode_img, "t": self.encode_text}
        index_dev = encode[index_enc](self.index_ds, self.index_field)
        test_dev = encode[test_enc](self.test_ds, self.test_field)
        self._index_dev, self._test_dev = index_dev, test_dev
        self.index_features, self.test_features = index_dev.cpu().numpy(), test_dev.cpu().numpy()
        if cache_file is not None:
            torch.save({"index_features": self.index_features, "test_features": self.test_features,
                        "meta_info": {"clip_model_name": self.clip_model_name, "mode": self.mode, "index_field": self.index_field,
                                      "test_field": self.test_field}}, cache_file)
        for name in ("vision_encoder", "text_encoder"):
            if hasattr(self, name):
                delattr(self, name)

    @torch.inference_mode()
    def encode_text(self, ds: Sequence[dict], text_field: str) -> torch.Tensor:
        """Every text of `ds` through the tokenizer and the tower, `batch_size` at a time: each batch is tokenized as the reference does
        (padded to its longest member), packed to its valid tokens and run in one pass -> (len(ds), dim) fp32 unit rows on the device."""
        n = len(ds)
        out = None
        for b0 in range(0, n, self.batch_size):
            texts = [ds[i][text_field] for i in range(b0, min(n, b0 + self.batch_size))]
            enc = self.tokenizer(texts, padding=True, return_tensors="pt", truncation=True)
            feats = self.text_encoder.encode(enc["input_ids"], enc["attention_mask"])
            if out is None:
                out = torch.empty((n, feats.shape[1]), dtype=torch.float32, device=feats.device)
            out[b0:b0 + len(texts)] = feats
        if out is None:
            raise ValueError("encode_text: empty dataset")
        return out

    def _pixel_values(self, images: list, pool) -> torch.Tensor:
        if self._img_processor is not None:
            return self._img_processor(images)
        from licv import frontend
        S = self.vision_encoder.arch.image_size
        if self.device_resize:
            rgb = [np.asarray((im if hasattr(im, "convert") else _to_pil(im)).convert("RGB")) for im in images]
            sizes, crops = [], []
            for a in rgb:
                (nw, nh), (left, top) = frontend.clip_resize_geometry(a.shape[1], a.shape[0], S)
                sizes.append((nh, nw))
                crops.append((top, left, S, S))
            return frontend.resize_images(rgb, sizes, crops, "bicubic", (S, S), normalize=(CLIP_MEAN, CLIP_STD), device=self.device)
        crop = lambda im: resize_center_crop_u8(im, S)
        u8 = np.stack(list(pool.map(crop, images)) if pool is not None else [crop(im) for im in images])
        return frontend.preprocess_images(torch.from_numpy(u8).to(self.device), mean=CLIP_MEAN, std=CLIP_STD)[0]

    @torch.inference_mode()
    def encode_img(self, ds: Sequence[dict], img_field: str) -> torch.Tensor:
        """Every image of `ds` through the tower, `batch_size` at a time, one pass per batch -> (len(ds), dim) fp32 unit rows on the
        device."""
        n = len(ds)
        out = None
        pool = ThreadPoolExecutor(self.num_workers) if self.num_workers > 0 else None
        try:
            for b0 in range(0, n, self.batch_size):
                images = [ds[i][img_field] for i in range(b0, min(n, b0 + self.batch_size))]
                feats = self.vision_encoder.encode(self._pixel_values(images, pool))
                if out is None:
                    out = torch.empty((n, feats.shape[1]), dtype=torch.float32, device=feats.device)
                out[b0:b0 + len(images)] = feats
        finally:
            if pool is not None:
                pool.shutdown()
        if out is None:
            raise ValueError("encode_img: empty dataset")
        return out

    # ------------------------------------------------------------------------------------------ search
    def retrieve(self, ice_num: int) -> List[List[int]]:
        """For every test row the `ice_num` index rows of largest inner product, best first (reversed_order: best last)."""
        from licv import ops
        if self._index_dev is None:                                      # features came from a cache file: the device is first touched here
            self._index_dev = torch.from_numpy(self.index_features).to(self.device)
            self._test_dev = torch.from_numpy(self.test_features).to(self.device)
        idx_list = ops.topk_ip(self._test_dev, self._index_dev, int(ice_num))[0].tolist()
        if self.reversed_order:
            idx_list = [list(reversed(i)) for i in idx_list]
        return idx_list
