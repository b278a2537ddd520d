"""The early form of the lazy route, host side: the rank table against the reference generator, and the cutoff policy."""
import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.pipeline_greedy import EarlyCutoff

FMTS = ["bf16", "bfp8", "bfp4", "bfp2"]


@pytest.mark.parametrize("tiles", [4, 128, 32768, 32769])
def test_rank_table_is_argsort_of_the_reference_permutation(tiles):
    # mixed_tile_greedy.py draws rng.permutation(candidates) once per format; while every tile is a candidate the third draw is the
    # visiting order of the last-but-one pass of a four-format search
    rng = np.random.default_rng(123)
    rng.permutation(tiles)
    rng.permutation(tiles)
    perm = rng.permutation(tiles)
    want = np.argsort(perm, kind="stable").astype(np.uint32)
    assert np.array_equal(hb.rank_table_host(perm), want)
    assert np.array_equal(hb.early_rank_host(123, tiles), want)
    # order 0 is the second draw
    rng = np.random.default_rng(7)
    rng.permutation(tiles)
    assert np.array_equal(hb.early_rank_host(7, tiles, which=0), np.argsort(rng.permutation(tiles), kind="stable").astype(np.uint32))


def test_first_batch_of_a_key_is_unpredicted_and_the_next_follows_it():
    pol = EarlyCutoff(0.02, 0.35)
    assert pol.cutoff(16384, FMTS, "pcc", 0.999, [123] * 8) == 0
    assert pol.learn(16384, FMTS, "pcc", 0.999, 123, 2532) == 2583          # ceil(2532 * 1.02) = ceil(2582.64)
    assert pol.cutoff(16384, FMTS, "pcc", 0.999, [123] * 8) == 2583
    pol.learn(16384, FMTS, "pcc", 0.999, 123, 1000)                         # only the previous batch counts
    assert pol.cutoff(16384, FMTS, "pcc", 0.999, [123]) == 1020
    pol.learn(16384, FMTS, "pcc", 0.999, 123, 0)
    assert pol.cutoff(16384, FMTS, "pcc", 0.999, [123]) == 0


def test_cutoff_is_capped_at_the_lazy_routes_listed_fraction():
    pol = EarlyCutoff(0.02, 0.35)
    assert pol.learn(128, FMTS, "pcc", 0.9, 5, 128) == 44                    # int(0.35 * 128)
    assert pol.cutoff(128, FMTS, "pcc", 0.9, [5, 5]) == 44


def test_keys_are_separate():
    pol = EarlyCutoff(0.0, 1.0)
    pol.learn(128, FMTS, "pcc", 0.999, 123, 30)
    assert pol.cutoff(128, FMTS, "pcc", 0.999, [123]) == 30
    assert pol.cutoff(256, FMTS, "pcc", 0.999, [123]) == 0
    assert pol.cutoff(128, FMTS[:3], "pcc", 0.999, [123]) == 0
    assert pol.cutoff(128, FMTS, "mae", 0.999, [123]) == 0
    assert pol.cutoff(128, FMTS, "pcc", 0.99, [123]) == 0
    assert pol.cutoff(128, FMTS, "pcc", 0.999, [124]) == 0


def test_off_when_the_seeds_of_a_batch_differ():
    pol = EarlyCutoff(0.0, 1.0)
    pol.learn(128, FMTS, "pcc", 0.999, 123, 30)
    assert pol.cutoff(128, FMTS, "pcc", 0.999, [123, 124]) == 0
    assert pol.cutoff(128, FMTS, "pcc", 0.999, [123, 123, 123]) == 30
    assert pol.cutoff(128, FMTS, "pcc", 0.999, []) == 0
