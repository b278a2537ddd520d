"""The whole-tensor pcc column against a plain float64 Pearson of (x, y) on the host routes: tile_search.columns_from_stats on the
emulation backend's records (bit-identical to the oracle's and K1's) and the emulation backend's random search against
oracle.random_search.  The moment form Σxy − n·x̄·ȳ over float32-rounded products is ill-conditioned on offset float32 tensors
(mean >> std); pipeline_common.moment_pcc_gate sends those to a centred float64 recomputation (DESIGN §2 "Float columns").

Contract of every case: |pcc − pcc64| <= 2.5e-7 where Σx², Σy² lie in [2^-92, 2^124]; mae within 1e-9·max(1, mae64); atol exactly
max|x − y|."""
import numpy as np
import pytest

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.mixed_tile_random import random_search, score_band
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import columns_from_stats, compute_tile_stats
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.pipeline_common import (PCC_F64_TOL, SUM_SQ_HI, SUM_SQ_LO, centred_pcc, columns_from_sums_batch,
                                                       moment_pcc_gate)

ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
RATIOS = (0.0, 3.0, 10.0, 100.0, 1e3, 1e4)   # mean / std
SHAPES = ((32, 32), (100, 72), (768,), (256, 512))


def bf16_values(x: np.ndarray) -> np.ndarray:
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def offset_tensor(shape, ratio: float, seed: int = 0, std: float = 0.02) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (ratio * std + std * rng.standard_normal(shape)).astype(np.float32)


def reference_columns(x: np.ndarray, amap: np.ndarray) -> tuple[float, float, float, np.ndarray]:
    """(pcc64, mae64, atol, y) of the oracle's reconstruction under a tile map."""
    x2d = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else None
    if x2d is None:   # a vector: the 2-D flatten pads it into rows of 32 (tile_utils.flatten_2d), pads are zeros in x and y
        n = x.size
        x2d = np.zeros((-(-n // 32), 32), dtype=np.float32)
        x2d.reshape(-1)[:n] = x
    th, tw = orc.tiles_hw(*x2d.shape)
    y2d = orc.apply_assignment(x2d, np.asarray(amap, dtype=np.int8).reshape(th, tw))
    xf, yf = x2d.reshape(-1)[: x.size], y2d.reshape(-1)[: x.size]
    d = np.abs(xf.astype(np.float64) - yf.astype(np.float64))
    return orc.pearson_corr_f64(xf, yf), float(d.mean()), float(np.max(np.abs(xf - yf))), yf


def check_columns(c: dict, x: np.ndarray, amap: np.ndarray, what: str) -> None:
    pcc64, mae64, atol, _y = reference_columns(x, amap)
    sx2, sy2 = c["sums"][1], c["sums"][3]
    if SUM_SQ_LO <= sx2 <= SUM_SQ_HI and SUM_SQ_LO <= sy2 <= SUM_SQ_HI:
        assert abs(c["pcc"] - pcc64) <= PCC_F64_TOL, f"{what}: pcc {c['pcc']!r} vs float64 {pcc64!r}"
    assert abs(c["mae"] - mae64) <= 1e-9 * max(1.0, mae64), f"{what}: mae {c['mae']!r} vs {mae64!r}"
    assert c["atol"] == atol, f"{what}: atol {c['atol']!r} vs {atol!r}"


def maps_for(ts, seed: int = 0) -> dict:
    rng = np.random.default_rng(seed)
    maps = {f: np.full(ts.tiles, MIXED_TILE_FORMATS.index(f), dtype=np.int8) for f in ALL}
    maps["random"] = rng.integers(0, 4, ts.tiles).astype(np.int8)
    return maps


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_columns_against_f64_pearson(shape, ratio, storage):
    x = offset_tensor(shape, ratio, seed=int(ratio) % 7)
    if storage == "bf16":
        x = bf16_values(x)
    ts = compute_tile_stats(x, ALL, Quantizer("emulation"))
    for name, amap in maps_for(ts).items():
        check_columns(columns_from_stats(ts, amap), x, amap, f"{storage} {shape} mean/std {ratio} map {name}")


def test_columns_of_searched_maps_1024():
    """The greedy and threshold plugins' own columns (meta["columns"]) on a 1024² offset float32 tensor."""
    from tests.test_golden_r2 import run_package_algo

    x = offset_tensor((1024, 1024), 100.0, seed=3)
    for name, params in (("mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": 5}),
                         ("mixed-tile-threshold", {"metric": "pcc", "threshold": 0.999}),
                         ("mixed-tile-random", {"metric": "pcc", "threshold": 0.999, "iters": 2, "seed": 5})):
        res = run_package_algo(name, params, x)
        check_columns(res.meta["columns"], x, res.meta["assignment"].reshape(-1), name)


def coherent_tensor(shape, seed: int = 9) -> np.ndarray:
    """An offset float32 tensor of four distinct values whose float32 squares all round down (the moment form's rounding errors add up
    instead of cancelling), at mean/std = 0.95: κx = 1 + 0.95^-2 ≈ 1.9, so the gate's first-order bound, 2^-24·(√(κx·κy) + (κx+κy)/2),
    sits just below PCC_F64_TOL and the moment column is kept.  Each value is the nearest float32 at or above 1 + σ·z, z = ±0.5, ±1.5
    over √1.25, whose square rounds down."""
    z = np.array([-1.5, -0.5, 0.5, 1.5]) / np.sqrt(1.25)
    vals = []
    for v in (1.0 + z / 0.95).astype(np.float32):
        while not float(v) ** 2 > float(v * v):
            v = np.nextafter(v, np.float32(4))
        vals.append(v)
    vals = np.asarray(vals, dtype=np.float32)
    assert np.unique(vals).size == 4 and np.all(vals.astype(np.float64) ** 2 > (vals * vals).astype(np.float64))
    return vals[np.random.default_rng(seed).integers(0, 4, shape)]


def test_coherent_tensor_below_the_gate():
    """The coherent tensor keeps its moment columns (the gate does not fire for any pure map) and they still meet the contract: the
    first-order bound holds where the rounding errors do not cancel."""
    x = coherent_tensor((256, 256))
    ts = compute_tile_stats(x, ALL, Quantizer("emulation"))
    for f in ALL:
        amap = np.full(ts.tiles, MIXED_TILE_FORMATS.index(f), dtype=np.int8)
        c = columns_from_stats(ts, amap)
        assert not moment_pcc_gate(np.asarray(c["sums"])[None], x.size, True)[0], f
        check_columns(c, x, amap, f"coherent {f}")


def test_columns_harder_cases():
    # a constant tensor (zero denominator on both sides: the rule of metrics.py), and the same with one outlier
    const = np.full((64, 96), 1.1, dtype=np.float32)
    outlier = const.copy()
    outlier[17, 33] = 1.3
    # y == x: the bf16 row of bf16-valued data
    same = bf16_values(offset_tensor((128, 160), 50.0, seed=4))
    coherent = coherent_tensor((256, 256))
    for what, x in (("constant", const), ("constant+outlier", outlier), ("y==x", same), ("coherent", coherent)):
        ts = compute_tile_stats(x, ALL, Quantizer("emulation"))
        for name, amap in maps_for(ts, 1).items():
            check_columns(columns_from_stats(ts, amap), x, amap, f"{what} map {name}")


def test_gate_regression_zero_mean_bit_identical():
    """Zero-mean float32 and bf16 tensors: the gate does not fire and the columns are the moment columns bit for bit."""
    for x in (offset_tensor((512, 512), 0.0, seed=1), bf16_values(offset_tensor((512, 512), 0.0, seed=2))):
        ts = compute_tile_stats(x, ALL, Quantizer("emulation"))
        for name, amap in maps_for(ts).items():
            c = columns_from_stats(ts, amap)
            assert not moment_pcc_gate(np.asarray(c["sums"])[None], x.size, True)[0], name
            want = hb.columns_from_sums(np.append(np.asarray(c["sums"]), c["atol"]), x.size)
            assert (c["pcc"], c["mae"], c["atol"]) == (want["pcc"], want["mae"], want["atol"]), name
            batch = columns_from_sums_batch(np.append(np.asarray(c["sums"]), c["atol"])[None], float(x.size))[0]
            assert np.array_equal(batch, [c["pcc"], c["mae"], c["atol"]]), name


def test_gate_definition():
    """bf16 storage never fires; outside the float32-safe range nothing fires; a degenerate side always fires inside it."""
    s = np.array([[1000.0, 1000.0 ** 2 / 1000 + 1e-3, 1000.0, 1000.0 + 1e-3, 1000.0, 0.0]])
    assert moment_pcc_gate(s, 1000.0, True)[0] and not moment_pcc_gate(s, 1000.0, False)[0]
    assert not moment_pcc_gate(s * 2.0 ** 130, 1000.0, True)[0]
    assert moment_pcc_gate(np.array([[10.0, 1.0, 10.0, 1.0, 1.0, 0.0]]), 100.0, True)[0]   # am2 = 0
    # centred_pcc's zero-denominator rule is the moment form's
    x = np.full(100, 0.1, dtype=np.float32)
    assert centred_pcc(x, x, [x.astype(np.float64).sum(), 0, x.astype(np.float64).sum(), 0, 0, 0.0], 100) == 1.0
    assert centred_pcc(x, x * 0 + 0.2, [x.astype(np.float64).sum(), 0, 20.0, 0, 0, 10.0], 100) == 0.0


# --------------------------------------------------------------------------------------------------------------- random search

def emulation_random(x, formats, threshold, iters, seed):
    ts = compute_tile_stats(x, formats, Quantizer("emulation"))
    a, samples, _n = random_search(ts, x, formats, "pcc", threshold, iters, seed, Quantizer("emulation"))
    return a, samples


def test_random_search_offset_selection():
    """The case of the issue: the moment pcc of this offset tensor's samples is ~1e-5 off the float32 score, outside the old band."""
    x = (1.0 + 1e-3 * np.random.default_rng(1).standard_normal((256, 512))).astype(np.float32)
    fmts = ["bf16", "bfp8"]
    a, _ = emulation_random(x, fmts, 0.26520971, 8, 7)
    want, _c, _s = orc.random_search(x, fmts, "pcc", 0.26520971, 8, 7)
    assert np.array_equal(a, want)


def test_random_search_adversarial_thresholds():
    """Thresholds between each sample's column and its float32 score (and one float32 ulp either side of the float32 score)."""
    x = (1.0 + 1e-3 * np.random.default_rng(2).standard_normal((128, 256))).astype(np.float32)
    fmts = ["bfp8", "bfp4", "bfp2"]
    _w, _c, ref_samples = orc.random_search(x, fmts, "pcc", 0.5, 4, 11)
    _a, samples = emulation_random(x, fmts, 0.5, 4, 11)
    tried = 0
    for s, r in zip(samples, ref_samples):
        f32 = np.float32(r["pcc"])
        for thr in {0.5 * (s["pcc"] + r["pcc"]), float(np.nextafter(f32, np.float32(2))), float(f32), float(np.nextafter(f32, np.float32(-2)))}:
            a, _ = emulation_random(x, fmts, thr, 4, 11)
            want, _c, _s = orc.random_search(x, fmts, "pcc", thr, 4, 11)
            assert np.array_equal(a, want), f"threshold {thr!r}"
            tried += 1
    assert tried >= 8


def test_score_band_model():
    assert score_band(1024) == 1e-5
    assert score_band(4096 * 4096) > 1.43e-4 * 2   # the measured float32-vs-float64 gap at 4096², with room


# --------------------------------------------------------------------------------------------------------------- bench tensors

def _gate_on_records(x: np.ndarray) -> list:
    """Maps whose column the gate would recompute on x AS IF it were stored in float32 (bf16 storage never fires: this is the stronger
    claim), from the column sums of the oracle's records of the whole matrix (bit-equal to K1's): each pure mixed-tile map and a random
    map.  → the names of the maps that fire."""
    recs = orc.tile_stats(x, ALL)
    slots = orc.mask_slots(orc.fmt_mask(ALL))
    rng = np.random.default_rng(0)
    maps = {f: np.full(recs.shape[0], MIXED_TILE_FORMATS.index(f)) for f in ALL}
    maps["random"] = rng.integers(0, 4, recs.shape[0])
    fired = []
    for name, a in maps.items():
        sel = np.asarray([2 + 5 * slots[f] for f in MIXED_TILE_FORMATS])[a]   # each tile's Σy column
        t = np.arange(recs.shape[0])
        sums = [recs[:, 0].sum(), recs[:, 1].sum(), recs[t, sel].sum(), recs[t, sel + 1].sum()]
        if moment_pcc_gate(np.asarray(sums)[None], float(x.size), True)[0]:
            fired.append(name)
    return fired


def test_gate_quiet_on_bench_tensors():
    """The gate fires on none of the tensors bench.py draws — even if they were stored in float32: a 4096² m1 tensor (bf16
    N(0, 0.02²)), the seven synthetic:llama3-8b layer-0 weights (bf16) and the five float32 synthetic:deepseek-r1-layer0 self_attn
    matrices, whole (its two layernorm vectors are bf16).  bench.py draws these on the device (other values of the same distributions); here they come from the CPU
    generator.  So the bench's columns stay the moment columns and its timed path never runs the centred recomputation."""
    import concurrent.futures as cf

    import torch

    from quantization_analysis_amd import model_source as ms
    from quantization_analysis_amd.pipeline_common import cpu_budget

    def m1():
        g = torch.Generator().manual_seed(0)
        return (torch.randn((4096, 4096), generator=g) * 0.02).to(torch.bfloat16)

    jobs = [("m1", m1)]
    for preset, query in (("synthetic:llama3-8b", "model.layers.0."), ("synthetic:deepseek-r1-layer0", "model.layers.0.self_attn")):
        index = ms.build_model_index(preset)
        for name in ms.resolve_selected_tensors(index, query):
            shape, dtype = index.shape_dtype(name)
            if len(shape) == 2:
                jobs.append((f"{preset} {name}", lambda index=index, name=name: index.load(name)))
            else:   # deepseek's two layernorm vectors (ones + 0.01·N, mean/std 100): bf16 storage, exact products, no gate
                assert dtype == "bf16", name

    def one(job):
        name, load = job
        t = load()
        assert t.dtype in (torch.bfloat16, torch.float32), name
        return name, _gate_on_records(t.float().numpy())

    with cf.ThreadPoolExecutor(max_workers=max(1, min(4, cpu_budget()))) as pool:   # the oracle's C code releases the GIL
        got = dict(pool.map(one, jobs))
    assert len(got) == 1 + 7 + 5
    assert all(v == [] for v in got.values()), {k: v for k, v in got.items() if v}
