"""The inputs of tests/test_threshold_metrics_gpu.py (the threshold search's device routes under mae and atol), and what those tests
rely on, checked without a GPU: at every threshold of the table the host route (K4 on the oracle's records + the literal re-scoring)
gives the literal float32 rule's map, every knife threshold really puts tiles inside the band and splits the map over several
formats, the 2^-60 input is knife-edge on every tile (the list overflows at any cap), and the 2^20 / 2^40 thresholds lie above 1
(band = KNIFE_BAND·|threshold|).

The band of these metrics is absolute below 1 (csrc/mtq_decide.hpp threshold_decide: width = band·max(1, |thr32|), no per-tile
widening): at weight scale mae scores are around 1e-4 and 2e-6 is a few percent of them."""
import numpy as np
import pytest

from tests.inputs import gen
from tests.test_threshold_band import degenerate_tensor, knife_thresholds, offset, oracle_maps, record_route, scaled

ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
METRICS = ("mae", "atol")
SCALES = (-60, -20, 0, 20, 40)
# Several-format maps at every knife threshold need more than two tiles (one ulp under the lower of two tiles' bfp8 scores both go to
# bf16; one tile holds one format), so the table's ragged matrix is 65x81 (nine tiles: edge tiles of a single row, of 17 columns, and
# the 1x17 corner) and its vector has 7000 elements (218 rows of 32 and one of 24: seven tiles, the last one 27 rows).  The 33x17
# matrix and the 1000-element vector are the SMALL cases: every condition but that one.
RAGGED_SHAPE = (65, 81)
VECTOR_N = 7000

# label → (seed → float32 host values, bf16 storage?).  Seeds: a batch of a case is the case at seed, seed + 1, ...
MAKERS = {**{f"2^{k}": ((lambda s, k=k: scaled(k, seed=s + 7000 + k, shape=(96, 160))), False) for k in SCALES},
          "heavy_f32": ((lambda s: gen("heavy_f32", s + 710, (100, 72))), False),
          "heavy_bf16": ((lambda s: gen("heavy_bf16", s + 720, (128, 256))), True),
          "offset": ((lambda s: offset(1.0, 0.01, (128, 256), s + 730)), False),
          "degenerate": ((lambda s: degenerate_tensor()), False),
          "ragged_65x81": ((lambda s: scaled(0, s + 740, RAGGED_SHAPE)), False),
          "vector": ((lambda s: scaled(0, s + 750, (VECTOR_N,))), False)}
SMALL = {"ragged_33x17": ((lambda s: scaled(0, s + 760, (33, 17))), False),
         "vector_1000": ((lambda s: scaled(0, s + 770, (1000,))), False)}


def make(label: str, seed: int = 0) -> np.ndarray:
    return {**MAKERS, **SMALL}[label][0](seed)


def cases():
    """(label, float32 host values, bf16 storage?)"""
    return [(label, make(label), bf16) for label, (_f, bf16) in {**MAKERS, **SMALL}.items()]


def vector_form(v: np.ndarray) -> np.ndarray:
    """A vector as the device routes take it: ceil(n/32) rows of 32, the last one zero-filled (its element count travels beside it)."""
    vm = np.zeros((-(-v.size // 32) * 32,), dtype=np.float32)
    vm[: v.size] = v
    return vm.reshape(-1, 32)


def thresholds(x: np.ndarray, metric: str):
    """(the knife thresholds, the far one): a bfp8 and a bfp4 tile's float32 score with one float32 ulp either side of each, and one
    threshold further than the band from every score (above four times the largest, at least 1: nothing is knife-edge there)."""
    scores, _ = oracle_maps(x, metric, [])
    finite = np.concatenate([s[np.isfinite(s)] for s in scores.values()])
    return knife_thresholds(scores, formats=["bfp8", "bfp4"], per_format=1), max(4.0 * float(finite.max()), 1.0)


def tile_count(x: np.ndarray) -> int:
    return int(oracle_maps(x, "atol", [0.0])[1][0].size)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("label", list(MAKERS) + list(SMALL))
def test_inputs_meet_what_the_gpu_tests_rely_on(label, metric):
    x = make(label)
    knife, far = thresholds(x, metric)
    assert len(knife) == 6
    _, wants = oracle_maps(x, metric, knife + [far])
    with np.errstate(all="ignore"):
        for thr, want in zip(knife + [far], wants):
            got, nk = record_route(x, metric, thr)
            assert np.array_equal(got, want), (label, metric, thr, int(np.sum(got != want)), want.size)
            if thr == far:
                assert nk == 0, (label, metric, thr, nk)
                continue
            assert nk >= 1, (label, metric, thr)
            if label not in SMALL:
                assert np.unique(want).size >= 2, (label, metric, thr, np.unique(want))
            if label == "2^-60" and metric == "mae":
                assert nk == want.size, (thr, nk, want.size)          # the all-knife case
            if label in ("2^20", "2^40"):
                assert thr > 1.0, (label, metric, thr)                 # the band scales with the threshold


def test_batches_of_a_case_differ():
    """A batch is the case at consecutive seeds: different tensors (the degenerate one aside, which is fixed)."""
    for label in list(MAKERS) + list(SMALL):
        if label != "degenerate":
            assert not np.array_equal(make(label, 0), make(label, 1)), label
    assert tile_count(make("vector")) == 7 and tile_count(make("ragged_65x81")) == 9
    assert tile_count(make("vector_1000")) == 1 and tile_count(make("ragged_33x17")) == 2
