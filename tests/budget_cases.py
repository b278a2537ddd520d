"""Adversarial tile error tables for the budget allocation (budget_maps.allocate and mtq_budget_allocate_device), shared by
tests/test_budget_alloc_host.py (which asserts each table has the property it is there for) and tests/test_budget_alloc_gpu.py (which
runs every one of them on the device).  A case is (table float64 [T, 4], candidate formats, bits); everything is deterministic."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_BYTES_PER_ELEM, MIXED_TILE_FORMATS, mixed_tile_total_bytes

ALL = list(MIXED_TILE_FORMATS)
COST = {f: 1024.0 * MIXED_TILE_BYTES_PER_ELEM[f] for f in ALL}


class Case(NamedTuple):
    table: np.ndarray
    formats: list
    bits: float


def budget_of(bits: float, tiles: int) -> float:
    """allocate's budget expression."""
    return float(bits) / 8.0 * 1024.0 * float(tiles)


def exact_bits(target_bytes: float, tiles: int) -> float:
    """The bits whose budget is target_bytes exactly; tiles must be a power of two (every operation is then a scaling by one)."""
    assert tiles & (tiles - 1) == 0
    bits = target_bytes * 8.0 / (1024.0 * tiles)
    assert budget_of(bits, tiles) == target_bytes and 0.0 < bits <= 16.0
    return bits


def taken(table, formats, bits):
    """(take, order, tiles, frm, to, slope): hull_segments' sorted steps and how many of them allocate took (its taken steps are a
    prefix: a step is taken when its tile's final point is at or past the step's)."""
    order, tiles, frm, to, slope = bm.hull_segments(np.asarray(table, dtype=np.float64), [f for f in ALL if f in formats])
    got = bm.allocate(table, formats, bits)
    assert not isinstance(got, str), got
    rank = np.array([order.index(f) if f in order else -1 for f in ALL])
    final = rank[got[0].reshape(-1).astype(np.int64)]
    took = to <= final[tiles]
    take = int(took.sum())
    assert took[:take].all() and not took[take:].any()
    return take, order, tiles, frm, to, slope


def random_table(seed: int, tiles: int) -> np.ndarray:
    """Errors that fall with the format's size, as real tables do, with a wide spread between tiles."""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(-12.0, 2.0, size=(tiles, 1)))
    steps = rng.uniform(0.0, 1.0, size=(tiles, 4))
    steps[:, 0] *= 1e-6
    return np.cumsum(steps, axis=1) * scale


def dyadic_table(tiles: int = 16384) -> np.ndarray:
    rng = np.random.default_rng(11)
    t = np.zeros((tiles, 4))
    t[:, 1] = rng.choice([0.125, 0.25], size=tiles)
    t[:, 2] = rng.choice([0.5, 1.0], size=tiles)
    t[:, 3] = rng.choice([2.0, 4.0, 8.0], size=tiles)
    return t


@functools.lru_cache(maxsize=None)
def dyadic_case() -> Case:
    """1: thousands of tiles share each slope; bits puts the cut strictly inside a group of equal slopes."""
    t = dyadic_table()
    for bits in np.arange(2.25, 15.9, 0.0625):
        take, _o, _t, _f, _to, slope = taken(t, ALL, float(bits))
        if 0 < take < slope.size and slope[take - 1] == slope[take]:
            return Case(t, ALL, float(bits))
    raise AssertionError("no budget cuts the dyadic table inside a group of equal slopes")


@functools.lru_cache(maxsize=None)
def twin_key_case() -> Case:
    """2: a tile whose two hull steps carry one key (collinear points: equal quotients, or the clamp), five tiles of steeper and five
    of flatter slopes around it, and a budget that takes the first of the two steps and not the second."""
    rng = np.random.default_rng(5)
    n = 20000
    e3 = rng.uniform(1.0, 2.0, n)
    s = rng.uniform(1e-4, 1e-3, n)
    e2 = e3 - s * (COST["bfp4"] - COST["bfp2"])
    e1 = e2 - s * (COST["bfp8"] - COST["bfp4"])
    pool = np.stack([e1, e1, e2, e3], axis=1)
    _order, tiles, _frm, _to, slope = bm.hull_segments(pool, ALL)
    twin = None
    for r in range(n):
        k = slope[tiles == r]
        if k.size == 2 and k[0] == k[1]:
            twin = r
            break
    assert twin is not None, "no tile with two steps of one key in the pool"
    steep = np.array([[0.0, 0.0, 0.0, 100.0 + i] for i in range(5)])       # one step bfp2 -> bfp4 each, far steeper
    flat = np.array([[0.0, 0.0, 0.0, 1e-9 * (i + 1)] for i in range(5)])   # far flatter
    t = np.concatenate([steep, pool[twin:twin + 1], flat])
    counts = {"bf16": 0, "bfp8": 0, "bfp4": 6, "bfp2": 5}                   # the steep steps and the twin's first
    bits = (mixed_tile_total_bytes(counts) + 100.0) * 8.0 / (1024.0 * t.shape[0])
    return Case(t, ALL, bits)


def equal_errors_case() -> Case:
    """3: bf16, bfp8 and bfp4 err alike: the cheapest of them, bfp4, is kept at any budget."""
    t = np.tile(np.array([[0.25, 0.25, 0.25, 3.0]]), (40, 1)) * np.arange(1, 41)[:, None]
    return Case(t, ALL, 16.0)


def above_hull_case(bits: float = 6.0) -> Case:
    """4: bfp8 lies above the chord from bfp4 to bf16: no tile ever takes it."""
    rng = np.random.default_rng(3)
    e2 = rng.uniform(1.0, 2.0, 300)
    chord = e2 * (COST["bf16"] - COST["bfp8"]) / (COST["bf16"] - COST["bfp4"])     # the chord's height at bfp8 when e(bf16) = 0
    t = np.stack([np.zeros(300), chord * 1.05, e2, e2 * 3.0], axis=1)
    return Case(t, ALL, bits)


def negative_subnormal_case() -> Case:
    """5: negative entries and subnormals (tables are sums of squares, but allocate takes any finite table)."""
    rng = np.random.default_rng(9)
    t = random_table(9, 500)
    t[::7] -= 5.0
    t[1::7] *= -1.0
    sub = 5e-324 * rng.integers(1, 1000, size=(60, 4)).astype(np.float64)
    t[2:422:7] = np.sort(sub, axis=1)
    t[3::50] = 0.0
    return Case(t, ALL, 5.0)


@functools.lru_cache(maxsize=None)
def exact_budget_case() -> Case:
    """10: the budget equals the size after a prefix exactly: that prefix is taken (allocate stops at size > budget, not >=)."""
    t = random_table(21, 256)
    take, order, tiles, frm, to, _slope = taken(t, ALL, 5.0)
    assert take > 10
    keep = take - 3
    cnt = {f: 0 for f in ALL}
    cnt[order[0]] = 256
    for i in range(keep):
        cnt[order[frm[i]]] -= 1
        cnt[order[to[i]]] += 1
    return Case(t, ALL, exact_bits(mixed_tile_total_bytes(cnt), 256))


def floor_case() -> Case:
    """11: the budget equals the all-cheapest size: a map is made and every tile stays at bfp2."""
    return Case(random_table(22, 128), ALL, exact_bits(mixed_tile_total_bytes({"bf16": 0, "bfp8": 0, "bfp4": 0, "bfp2": 128}), 128))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name → Case, every one of them with a finite table and a budget at or above the floor (allocate returns a map)."""
    return {
        "dyadic_cut_inside_group": dyadic_case(),
        "twin_key_cut_between": twin_key_case(),
        "equal_errors": equal_errors_case(),
        "above_hull": above_hull_case(),
        "above_hull_tight": above_hull_case(3.0),
        "negative_subnormal": negative_subnormal_case(),
        "two_formats": Case(random_table(31, 300), ["bfp8", "bfp2"], 4.0),
        "three_formats": Case(random_table(32, 300), ["bf16", "bfp4", "bfp2"], 6.5),
        "three_formats_listed_out_of_order": Case(random_table(33, 300), ["bfp4", "bf16", "bfp8"], 9.0),
        "one_format": Case(random_table(34, 50), ["bfp4"], 9.0),
        "one_tile": Case(random_table(41, 1), ALL, 8.8),
        "tiles_257": Case(random_table(42, 257), ALL, 4.5),
        "tiles_70000": Case(random_table(43, 70000), ALL, 4.25),
        "exact_budget": exact_budget_case(),
        "floor": floor_case(),
        "above_all_bf16": Case(random_table(51, 200), ["bfp8", "bfp4", "bfp2"], 16.0),
        "all_bf16_exactly": Case(random_table(52, 200), ALL, 16.0),
    }


def below_floor_case() -> Case:
    """13: a budget below the all-bfp2 size."""
    return Case(random_table(61, 64), ALL, 1.0)


def nan_case() -> Case:
    """14: a NaN in a column that is not a candidate still refuses the table."""
    t = random_table(62, 64)
    t[17, 0] = np.nan
    return Case(t, ["bfp8", "bfp4", "bfp2"], 6.0)


def inf_case() -> Case:
    t = random_table(63, 64)
    t[40, 3] = np.inf
    return Case(t, ALL, 6.0)


def refused_cases() -> dict:
    """name → (Case, status of mtq_budget_allocate_device)."""
    return {"below_floor": (below_floor_case(), 1), "nan_outside_candidates": (nan_case(), 2), "inf": (inf_case(), 2)}


def split(tiles: int, parts: int) -> np.ndarray:
    """seg_first of `parts` uneven segments over `tiles` tiles (some empty when tiles < parts): int64 [parts + 1]."""
    if parts == 1:
        return np.array([0, tiles], dtype=np.int64)
    rng = np.random.default_rng(1000 + parts)
    cuts = np.sort(rng.integers(0, tiles + 1, size=parts - 1))
    return np.concatenate([[0], cuts, [tiles]]).astype(np.int64)


def segment_bits(bits: float, parts: int) -> list:
    """Per-segment bits around the case's: each segment gets a budget of its own."""
    return [float(min(16.0, max(0.5, bits + 0.37 * ((j % 5) - 2)))) for j in range(parts)]
