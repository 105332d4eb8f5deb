"""ops.pack_rows_plan: the gate that decides, on the host, whether a right-padded slice runs its language stack on packed rows, and
the cu_seqlens it hands to the native runner.  Host arithmetic only (licv_gemm_splitk_plan touches no device)."""
from licv import ops
from licv.config import IDEFICS_9B, IDEFICS_MID


def _shapes(arch):
    H, I = arch.hidden_size, arch.intermediate_size
    return [(3 * H, H), (H, H), (2 * I, H), (H, I)]


ONE = lambda M, N, K: 1
HEADLINE = [781, 740, 735, 788, 759, 775, 768, 723]          # synth_vqa_batch(IDEFICS_9B, 8, 800, 32, seed=426): real tokens of S = 800


def test_headline_slices_pack_to_twelve_row_tiles_each():
    tiles = lambda m: (m + 255) // 256
    assert sum(HEADLINE) == 6069 and tiles(4 * 800) == 13
    for lens, total in ((HEADLINE[:4], 3044), (HEADLINE[4:], 3025)):
        cu = ops.pack_rows_plan(lens, 800, _shapes(IDEFICS_9B))             # the library's own split-K plan
        assert cu is not None and cu[0] == 0 and cu[-1] == total and tiles(cu[-1]) == 12
        assert [b - a for a, b in zip(cu, cu[1:])] == lens
    # one stream: 25 tiles -> 24
    cu = ops.pack_rows_plan(HEADLINE, 800, _shapes(IDEFICS_9B))
    assert cu is not None and tiles(8 * 800) == 25 and tiles(cu[-1]) == 24


def test_cu_seqlens_are_the_running_sum_of_the_lengths():
    assert ops.pack_rows_plan([300, 1, 320, 200], 320, [], ONE) == [0, 300, 301, 621, 821]


def test_gate_needs_a_dropped_tile_and_512_rows():
    assert ops.pack_rows_plan([320, 320, 320, 300], 320, [], ONE) is None          # 1260 rows: still 5 tiles of 5
    assert ops.pack_rows_plan([320, 320, 320, 64], 320, [], ONE) == [0, 320, 640, 960, 1024]      # exactly 4 tiles of 5
    assert ops.pack_rows_plan([320, 320, 320, 65], 320, [], ONE) is None           # one row into the fifth tile
    assert ops.pack_rows_plan([255, 256], 400, [], ONE) is None                    # 511 rows: below the runner's large-batch route
    assert ops.pack_rows_plan([256, 256], 400, [], ONE) == [0, 256, 512]
    assert ops.pack_rows_plan([96, 96], 96, [], ONE) is None                       # nothing to drop


def test_gate_refuses_lengths_outside_the_rows():
    assert ops.pack_rows_plan([0, 600], 700, [], ONE) is None
    assert ops.pack_rows_plan([701, 600], 700, [], ONE) is None
    assert ops.pack_rows_plan([], 700, [], ONE) is None


def test_gate_keeps_the_split_k_plan_of_every_projection():
    asked = []

    def splits(M, N, K):
        asked.append((M, N, K))
        return 2 if (M < 1100 and N == 7) else 1
    shapes = [(5, 16), (7, 16), (9, 16)]
    assert ops.pack_rows_plan([500, 500], 640, shapes, splits) is None             # (1000, 7, 16) splits, (1280, 7, 16) does not
    assert (1000, 7, 16) in asked and (1280, 7, 16) in asked
    assert ops.pack_rows_plan([500, 500], 640, [(5, 16), (9, 16)], splits) == [0, 500, 1000]
    assert ops.pack_rows_plan([560, 560], 700, shapes, splits) == [0, 560, 1120]   # both sides of the plan agree again


def test_mid_model_shapes_open_the_gate_for_a_ragged_slice():
    assert ops.pack_rows_plan([200, 220, 288, 296], 320, _shapes(IDEFICS_MID)) == [0, 200, 420, 708, 1004]
