"""bench.py --dump-outputs without a GPU: which arrays a forward step's logits become, that the sample is fixed from run to run
and covers real tokens only, the dtypes written, and the 64 MB bound at the headline shape."""
import numpy as np
import torch

import bench                                  # the repository root is on sys.path (tests/conftest.py)
from licv.config import IDEFICS_MID, idefics_arch
from licv.synthetic import synth_vqa_batch


def test_forward_logits_dump_is_a_fixed_sample_of_real_token_rows(tmp_path):
    arch = IDEFICS_MID
    B, S = 4, 96
    batch = synth_vqa_batch(arch, B, S, 5, seed=426, min_len=80)
    V = arch.vocab_size + arch.additional_vocab_size
    out = torch.randn(B, S, V, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    bench.dump_outputs(tmp_path / "a", bench.step_outputs(out, batch, None))
    bench.dump_outputs(tmp_path / "b", bench.step_outputs(out, batch, None))
    got = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert sorted(got) == ["logits_last", "logits_sample", "logits_sample_rows"]
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
    rows = got["logits_sample_rows"]
    assert rows.dtype == np.float64 and len(rows) == min(bench.DUMP_LOGIT_ROWS, int(batch["attention_mask"].sum()))
    idx = torch.from_numpy(rows.astype(np.int64))
    assert bool(batch["attention_mask"].reshape(-1)[idx].all())
    assert got["logits_sample"].dtype == np.float32
    assert np.array_equal(got["logits_sample"], out.float().reshape(B * S, V)[idx].numpy())
    last = batch["attention_mask"].sum(1) - 1
    assert np.array_equal(got["logits_last"], out.float()[torch.arange(B), last].numpy())


def test_generate_rows_are_written_exactly_and_the_headline_dump_fits(tmp_path):
    seq = torch.tensor([[1, 32001, 7], [1, 5, 2]])
    bench.dump_outputs(tmp_path, bench.step_outputs(seq, None, None))
    got = np.load(tmp_path / "sequences.npy")
    assert got.dtype == np.float64 and np.array_equal(got, seq.numpy())
    arch = idefics_arch("idefics-9b")
    _, B, _, _, _ = bench.WORKLOADS["idefics9b_32shot_bs8"]
    V = arch.vocab_size + arch.additional_vocab_size
    assert (bench.DUMP_LOGIT_ROWS + B) * V * 4 + bench.DUMP_LOGIT_ROWS * 8 <= 64 * 2**20
