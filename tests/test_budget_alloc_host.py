"""The adversarial tables of tests/budget_cases.py have the properties they are there for (checked with budget_maps.hull_segments and
allocate on the host), and the mixed-tile-budget algorithm: registry, parameter checks, emulation run() = allocate on the emulation
table, and the reasons the hip route rebuilds from the device status."""
from __future__ import annotations

import numpy as np
import pytest

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms import ALGORITHM_REGISTRY, BUDGET_ALGORITHMS, create_algorithm
from quantization_analysis_amd.compression_algorithms import mixed_tile_budget as mtb
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import columns_from_stats, compute_tile_stats
from quantization_analysis_amd.compression_algorithms.tile_utils import mixed_tile_total_bytes
from tests import budget_cases as bc

ALL = bc.ALL


def _codes(case):
    got = bm.allocate(*case)
    assert not isinstance(got, str), got
    return got[0].reshape(-1), got[1], got[2]


def test_every_case_is_finite_and_gets_a_map():
    for name, case in bc.cases().items():
        assert np.all(np.isfinite(case.table)) and case.table.shape[1] == 4, name
        a, counts, size = _codes(case)
        assert a.shape == (case.table.shape[0],) and sum(counts.values()) == a.size, name
        assert size <= bc.budget_of(case.bits, a.size), name
        assert set(np.unique(a)) <= {ALL.index(f) for f in case.formats}, name


def test_dyadic_cut_falls_inside_a_group_of_equal_slopes():
    case = bc.dyadic_case()
    take, _order, tiles, _frm, _to, slope = bc.taken(*case)
    assert np.unique(case.table).size <= 8
    assert 0 < take < slope.size and slope[take - 1] == slope[take]
    assert np.count_nonzero(slope == slope[take]) > 1000          # thousands of tiles on the cut's slope
    assert tiles[take - 1] < tiles[take]                          # inside the group the order is by tile


def test_twin_key_tile_is_cut_between_its_two_steps():
    case = bc.twin_key_case()
    take, _order, tiles, _frm, to, slope = bc.taken(*case)
    assert tiles[take - 1] == tiles[take] == 5 and slope[take - 1] == slope[take]    # one tile, one key, the cut between its steps
    assert to[take - 1] < to[take]
    a, _counts, _size = _codes(case)
    assert a[5] == ALL.index("bfp4")


def test_equal_errors_keep_the_cheaper_format():
    a, counts, _size = _codes(bc.equal_errors_case())
    assert np.all(a == ALL.index("bfp4")) and counts["bf16"] == counts["bfp8"] == 0


def test_a_point_above_the_hull_is_skipped():
    for case in (bc.above_hull_case(), bc.above_hull_case(3.0), bc.above_hull_case(16.0)):
        order, _tiles, _frm, to, _slope = bm.hull_segments(case.table, ALL)
        assert not np.any(to == order.index("bfp8"))
        a, counts, _size = _codes(case)
        assert counts["bfp8"] == 0
    assert _codes(bc.above_hull_case())[1]["bf16"] > 0 and _codes(bc.above_hull_case())[1]["bfp4"] > 0


def test_negative_and_subnormal_entries():
    case = bc.negative_subnormal_case()
    t = case.table
    assert t.min() < 0.0 and np.any((t > 0.0) & (t < 2.2250738585072014e-308)) and np.any(t == 0.0)
    a, counts, _size = _codes(case)
    assert len([c for c in counts.values() if c]) >= 3
    _order, _tiles, _frm, _to, slope = bm.hull_segments(t, ALL)
    assert slope.min() >= 0.0 and np.any(slope == 0.0)           # a subnormal gain underflows to a key of +0


def test_candidate_subsets_and_sizes():
    cs = bc.cases()
    assert len(cs["two_formats"].formats) == 2 and len(cs["three_formats"].formats) == 3
    assert cs["one_tile"].table.shape[0] == 1 and cs["tiles_257"].table.shape[0] == 257 and cs["tiles_70000"].table.shape[0] == 70000
    for name in ("two_formats", "three_formats", "tiles_257", "tiles_70000"):
        _a, counts, _size = _codes(cs[name])
        assert len([c for c in counts.values() if c]) >= 2, name


def test_exact_budget_takes_the_step_that_lands_on_it():
    case = bc.exact_budget_case()
    _a, _counts, size = _codes(case)
    assert size == bc.budget_of(case.bits, 256)                   # > not >=: the prefix whose size equals the budget is taken


def test_budget_at_the_floor_and_above_everything():
    a, counts, size = _codes(bc.floor_case())
    assert np.all(a == ALL.index("bfp2")) and size == bc.budget_of(bc.floor_case().bits, 128)
    cs = bc.cases()
    take, _order, _tiles, _frm, _to, slope = bc.taken(*cs["above_all_bf16"])
    assert take == slope.size and _codes(cs["above_all_bf16"])[2] < bc.budget_of(16.0, 200)
    take, _order, _tiles, _frm, _to, slope = bc.taken(*cs["all_bf16_exactly"])
    assert take == slope.size and np.all(_codes(cs["all_bf16_exactly"])[0] == 0)


def test_refusals_and_the_reasons_rebuilt_from_the_status():
    for name, (case, status) in bc.refused_cases().items():
        reason = bm.allocate(*case)
        assert isinstance(reason, str), name
        assert mtb.status_reason(status, case.formats, case.bits, case.table.shape[0]) == reason, name
    assert "below the all-bfp2 size" in bm.allocate(*bc.below_floor_case())
    assert bm.allocate(*bc.nan_case()) == "the tile error table holds a non-finite value"
    assert mtb.status_reason(0, ALL, 4.0, 10) is None


def test_splits_cover_the_tiles_unevenly():
    for tiles in (1, 257, 70000):
        for parts in (1, 3, 64):
            first = bc.split(tiles, parts)
            assert first.shape == (parts + 1,) and first[0] == 0 and first[-1] == tiles and np.all(np.diff(first) >= 0)
    assert len(set(np.diff(bc.split(4096, 64)).tolist())) > 8
    empty = bm.allocate(np.zeros((0, 4)), ALL, 4.0)                # an empty segment: an empty map
    assert not isinstance(empty, str) and empty[0].size == 0 and empty[2] == 0.0


def test_registry_and_parameter_checks():
    assert BUDGET_ALGORITHMS == {"mixed-tile-budget": mtb.MixedTileBudgetCompression} and "mixed-tile-budget" not in ALGORITHM_REGISTRY
    with pytest.raises(ValueError, match="mixed-tile-budget"):                 # the list of known names holds it
        create_algorithm("nope")
    algo = create_algorithm("Mixed-Tile-Budget", {"bits": 4.5})
    assert algo.name == "mixed-tile-budget" and algo.bits == 4.5 and algo.scope == "tensor" and algo.metric == "pcc"
    assert create_algorithm("mixed-tile-budget", {"bits": 16, "scope": "model"}).scope == "model"
    for bits in (0, -1.0, 16.5, float("nan")):
        with pytest.raises(ValueError, match="bits per weight"):
            create_algorithm("mixed-tile-budget", {"bits": bits})
    with pytest.raises(ValueError, match="bits"):
        create_algorithm("mixed-tile-budget", {})
    with pytest.raises(ValueError, match="scope"):
        create_algorithm("mixed-tile-budget", {"bits": 4, "scope": "layer"})
    with pytest.raises(ValueError, match="metric"):
        create_algorithm("mixed-tile-budget", {"bits": 4, "metric": "mse"})
    with pytest.raises(ValueError, match="row layout only"):
        create_algorithm("mixed-tile-budget", {"bits": 4, "layout": "transpose"})
    with pytest.raises(ValueError, match="requires at least one of"):
        create_algorithm("mixed-tile-budget", {"bits": 4}).candidates(["mxfp4"])
    with pytest.raises(ValueError, match="pack_model"):
        create_algorithm("mixed-tile-budget", {"bits": 4, "scope": "model"}).run(np.zeros((32, 32), np.float32), ALL, Quantizer("emulation"), None)


def _weights(shape, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(shape).astype(np.float32) * 0.05
    w.reshape(-1)[::97] *= 30.0
    return w


@pytest.mark.parametrize("shape,bits,formats", [((96, 160), 4.5, ALL), ((70, 100), 3.0, ALL), ((70, 100), 9.0, ["bf16", "bfp8", "bfp4"]),
                                                ((1000,), 5.0, ALL), ((3, 40, 50), 6.0, ALL)])
def test_emulation_run_equals_allocate_on_the_emulation_table(tmp_path, shape, bits, formats):
    w = _weights(shape, seed=len(shape))
    q = Quantizer("emulation")
    algo = create_algorithm("mixed-tile-budget", {"bits": bits, "formats": formats})
    res = algo.run(w, ["bf16", "bfp8", "bfp4", "bfp2", "mxfp4"], q, CacheContext(tmp_path, "t", "emulation", False, "t"))
    assert len(res) == 1 and res[0].fmt == "MIXED" and res[0].compression == "mixed-tile-budget"
    ts = compute_tile_stats(w, formats, q)
    table = bm.tile_error_tables_emulation(ts.x2d, np.zeros((ts.tiles_w, 32, 32)))[1]
    want_a, want_counts, want_bytes = bm.allocate(table, formats, bits, (ts.tiles_h, ts.tiles_w))
    r = res[0]
    assert np.array_equal(r.meta["assignment"], want_a) and r.meta["assignment"].dtype == np.int8
    assert r.tile_counts == want_counts and r.tile_bytes == want_bytes == mixed_tile_total_bytes(want_counts)
    assert r.tile_bytes <= r.meta["budget_bytes"] == bc.budget_of(bits, ts.tiles)
    assert r.meta["tile_formats"] == formats and r.meta["bits"] == bits
    assert r.meta["predicted_sse"] == bm.predicted_sse(table, want_a)
    assert r.meta["columns"] == columns_from_stats(ts, want_a)
    assert np.asarray(r.y).shape == w.shape
    # predicted_sse is the map's weight-space squared error
    assert np.isclose(float(((np.asarray(r.y, np.float64) - w.astype(np.float64)) ** 2).sum()), r.meta["predicted_sse"], rtol=1e-9)


def test_emulation_run_raises_allocates_reason(tmp_path):
    algo = create_algorithm("mixed-tile-budget", {"bits": 1.0})
    with pytest.raises(ValueError, match="below the all-bfp2 size"):
        algo.run(_weights((64, 64)), ALL, Quantizer("emulation"), CacheContext(tmp_path, "t", "emulation", False, "t"))


def test_the_new_entries_are_bound_and_check_their_arguments_before_a_device():
    L = hb.lib()
    for name in ("mtq_tile_sq_error_batched", "mtq_budget_allocate_scratch_bytes", "mtq_budget_allocate_device"):
        assert name in hb.OPTIONAL_EXPORTS and hasattr(L, name)
    assert hb.MTQ_VERSION == 143 and L.mtq_version() == 143          # optional symbols: found by name, the number stays
    need = hb.budget_allocate_scratch_bytes(1000, 3)
    assert need >= 1000 * 25 and hb.budget_allocate_scratch_bytes(0, 3) == 0
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16                    # a host address: no check may dereference it
    INVALID = -1
    ok = dict(table=p, tiles=1000, first=p, n_seg=3, mask=0xF, budget=p, map=p, counts=p, status=p, scratch=p, nbytes=need)

    def call(**kw):
        a = {**ok, **kw}
        return L.mtq_budget_allocate_device(a["table"], a["tiles"], a["first"], a["n_seg"], a["mask"], a["budget"], a["map"], a["counts"],
                                            a["status"], a["scratch"], a["nbytes"], None)

    for bad in ({"table": None}, {"first": None}, {"budget": None}, {"map": None}, {"counts": None}, {"status": None}, {"scratch": None},
                {"n_seg": 0}, {"n_seg": -2}, {"tiles": 0}, {"mask": 0}, {"mask": 0x30}, {"nbytes": need - 1}, {"scratch": p + 4}):
        assert call(**bad) == INVALID, bad
        assert L.mtq_last_error()
    for args in ((None, 0, 3, 96 * 160, 96, 160, 160, p), (p, 0, 3, 96 * 160, 96, 160, 160, None), (p, 7, 3, 96 * 160, 96, 160, 160, p),
                 (p, 0, 0, 96 * 160, 96, 160, 160, p), (p, 0, 3, 96 * 160, 0, 160, 160, p), (p, 0, 3, 96 * 160, 96, 160, 128, p),
                 (p, 0, 3, 100, 96, 160, 160, p)):
        assert L.mtq_tile_sq_error_batched(*args, None) == INVALID, args
