"""Every hip route that reports a whole-tensor pcc column, against a plain float64 Pearson of (x, y) with y the oracle's reconstruction
(bit-equal to K2 / K3 and the proxy quantiser), on offset float32 tensors where the moment form is ill-conditioned, and the regression
guard: on zero-mean tensors the columns stay bit-identical to the moment columns of the same sums (DESIGN §2 "Float columns")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.pipeline_common import PCC_F64_TOL
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.test_columns_conditioning_host import ALL, RATIOS, bf16_values, coherent_tensor, offset_tensor, reference_columns
from tests.test_golden_r2 import run_package_algo

pytestmark = pytest.mark.gpu

PROXIES = ["mxfp4", "nvfp4"]
SHAPES = ((32, 32), (100, 72), (768,), (256, 512), (1024, 1024))


def dev(x: np.ndarray, bf16: bool):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def pcc_ok(got: float, x: np.ndarray, y: np.ndarray, what: str) -> None:
    want = orc.pearson_corr_f64(x.reshape(-1), y.reshape(-1))
    assert abs(got - want) <= PCC_F64_TOL, f"{what}: pcc {got!r} vs float64 {want!r}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_none_rows(shape, ratio, bf16):
    """cli._none_rows_hip: the pure mixed-tile formats (K1 records) and the mxfp4 / nvfp4 proxies (FP4P sums)."""
    from quantization_analysis_amd.cli import _none_rows_hip
    from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer

    x = offset_tensor(shape, ratio, seed=5)
    if bf16:
        x = bf16_values(x)
    cols = _none_rows_hip(dev(x, bf16), ALL + PROXIES, Quantizer("hip"))
    for f in ALL + PROXIES:
        if f in MIXED_TILE_FORMATS:
            pcc64, mae64, atol, y = reference_columns(x, np.full(_tiles(x), MIXED_TILE_FORMATS.index(f), dtype=np.int8))
        else:
            y = quantize_weight_values(x, f)
            atol = float(np.max(np.abs(x - y)))
            mae64 = float(np.abs(x.astype(np.float64) - y).mean())
        pcc_ok(cols[f][0], x, y, f"{shape} {ratio} {f}")
        assert abs(cols[f][1] - mae64) <= 1e-9 * max(1.0, mae64) and cols[f][2] == atol, f


def _tiles(x: np.ndarray) -> int:
    h, w = (x.reshape(-1, x.shape[-1]).shape if x.ndim > 1 else (-(-x.size // 32), 32))
    return int(np.prod(orc.tiles_hw(h, w)))


@pytest.mark.parametrize("layout", ("rows", "transpose"))
@pytest.mark.parametrize("ratio", (0.0, 100.0))
def test_plugins(layout, ratio):
    """The greedy / threshold / random plugins' meta["columns"] and the transpose plugin's rows, against the oracle's reconstruction
    under the plugin's map (over Xᵀ's grid in the transposed layout)."""
    x = offset_tensor((256, 512), ratio, seed=6)
    xs = np.ascontiguousarray(x.T) if layout == "transpose" else x
    for name, params in (("mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": 5}),
                         ("mixed-tile-threshold", {"metric": "pcc", "threshold": 0.999}),
                         ("mixed-tile-random", {"metric": "pcc", "threshold": 0.999, "iters": 3, "seed": 5})):
        res = run_package_algo(name, {**params, "layout": layout}, dev(x, False), backend="hip")
        pcc_ok(res.meta["columns"]["pcc"], xs, orc.apply_assignment(xs, res.meta["assignment"]), f"{name} {layout}")
    if layout == "transpose":
        from quantization_analysis_amd.compression_algorithms.transpose import _columns_hip

        cols = _columns_hip(dev(x, False), ALL + PROXIES)
        xt = np.ascontiguousarray(x.T)
        for f in ALL + PROXIES:
            y = quantize_weight_values(xt, f)
            pcc_ok(cols[f]["pcc"], xt, y, f"transpose {f}")


@pytest.mark.parametrize("scan", ("device", "host"))
def test_greedy_pipeline(scan):
    from quantization_analysis_amd.pipeline import GreedyPipeline

    xs = np.stack([offset_tensor((128, 256), r, seed=7 + i) for i, r in enumerate((0.0, 100.0, 1e3))])
    with GreedyPipeline(ALL, "pcc", 0.999, 123, chunk=3, pure_formats=ALL, scan=scan) as pipe:
        out = pipe.run(dev(xs, False))
    for i, r in enumerate(out):
        _p, _m, _a, y = reference_columns(xs[i], r.assignment.reshape(-1))
        pcc_ok(r.pcc, xs[i], y, f"{scan} tensor {i}")
        for f in ALL:
            pcc_ok(r.pure[f][0], xs[i], quantize_weight_values(xs[i], f), f"{scan} tensor {i} pure {f}")


def test_threshold_pipeline_run_and_ragged():
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    a = np.stack([offset_tensor((128, 256), r, seed=8 + i) for i, r in enumerate((0.0, 100.0))])
    b = np.stack([offset_tensor((96, 160), 1e3, seed=12)])
    v = offset_tensor((1000,), 100.0, seed=13)
    vm = np.zeros((32 * 32,), dtype=np.float32)
    vm[:1000] = v
    batches = [(dev(a, False), None), (dev(b, False), None), (dev(vm, False).view(1, 32, 32), 1000)]
    with ThresholdPipeline(ALL, "pcc", 0.999, chunk=2, pure_formats=ALL) as pipe:
        got = pipe.run_batches(batches)
        single = pipe.run(*batches[0])
    for xs, n, res in ((a, None, got[0]), (b, None, got[1]), (vm.reshape(1, 32, 32), 1000, got[2]), (a, None, single)):
        for i, r in enumerate(res):
            x = xs[i].reshape(-1)[: n or xs[i].size]
            y = orc.apply_assignment(xs[i], r.assignment).reshape(-1)[: x.size]
            pcc_ok(r.pcc, x, y, f"threshold {xs.shape} {i}")
            for f in ALL:
                yq = quantize_weight_values(xs[i], f).reshape(-1)[: x.size]
                pcc_ok(r.pure[f][0], x, yq, f"threshold {xs.shape} {i} pure {f}")


def test_coherent_and_constant():
    from quantization_analysis_amd.cli import _none_rows_hip
    from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer

    const = np.full((64, 96), 1.1, dtype=np.float32)
    outlier = const.copy()
    outlier[17, 33] = 1.3
    for what, x in (("coherent", coherent_tensor((256, 256))), ("constant", const), ("outlier", outlier)):
        cols = _none_rows_hip(dev(x, False), ALL + PROXIES, Quantizer("hip"))
        for f in ALL + PROXIES:
            pcc_ok(cols[f][0], x, quantize_weight_values(x, f), f"{what} {f}")


def test_random_search_equals_oracle():
    """hip mixed-tile-random against oracle.random_search: the offset tensor of the host test, and zero-mean 4096² float32 / bf16
    tensors with the threshold inside a sample's float32-vs-float64 gap."""
    x = (1.0 + 1e-3 * np.random.default_rng(1).standard_normal((256, 512))).astype(np.float32)
    res = run_package_algo("mixed-tile-random", {"metric": "pcc", "threshold": 0.26520971, "iters": 8, "seed": 7, "formats": "bf16,bfp8"},
                           dev(x, False), backend="hip")
    want, _c, _s = orc.random_search(x, ["bf16", "bfp8"], "pcc", 0.26520971, 8, 7)
    assert np.array_equal(res.meta["assignment"], want)
    for bf16 in (False, True):
        xl = offset_tensor((4096, 4096), 0.0, seed=21)
        if bf16:
            xl = bf16_values(xl)
        _w, _c, samples = orc.random_search(xl, ["bfp8", "bfp2"], "pcc", 0.5, 2, 3)
        y_pcc = samples[1]["pcc"]
        for thr in (float(np.nextafter(np.float32(y_pcc), np.float32(2))), float(y_pcc)):
            res = run_package_algo("mixed-tile-random", {"metric": "pcc", "threshold": thr, "iters": 2, "seed": 3, "formats": "bfp8,bfp2"},
                                   dev(xl, bf16), backend="hip")
            want, _c, _s = orc.random_search(xl, ["bfp8", "bfp2"], "pcc", thr, 2, 3)
            assert np.array_equal(res.meta["assignment"], want), (bf16, thr)


def test_zero_mean_columns_bit_identical():
    """The gate does not fire on zero-mean bf16 / float32 tensors: the columns equal hb.columns_from_sums of the same sums bit for bit."""
    from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
    from quantization_analysis_amd.compression_algorithms.tile_search import columns_from_stats, compute_tile_stats

    for bf16 in (False, True):
        x = offset_tensor((512, 512), 0.0, seed=30 + bf16)
        ts = compute_tile_stats(dev(x, bf16), ALL, Quantizer("hip"))
        for f in ALL:
            c = columns_from_stats(ts, np.full(ts.tiles, MIXED_TILE_FORMATS.index(f), dtype=np.int8))
            w = hb.columns_from_sums(np.append(np.asarray(c["sums"]), c["atol"]), float(x.size))
            assert (c["pcc"], c["mae"], c["atol"]) == (w["pcc"], w["mae"], w["atol"]), (bf16, f)


def test_fp4_proxy_columns_batched():
    """hb.fp4_proxy_columns over a (count, rows, cols) batch (the streamed driver's form): each matrix's proxy columns."""
    xs = np.stack([offset_tensor((96, 160), r, seed=40 + i) for i, r in enumerate((0.0, 100.0, 1e3))])
    got = hb.fp4_proxy_columns(dev(xs, False), PROXIES)
    for i, cols in enumerate(got):
        for f in PROXIES:
            pcc_ok(cols[f][0], xs[i], quantize_weight_values(xs[i], f), f"batched {f} matrix {i}")


def test_greedy_pipeline_run_batches():
    """GreedyPipeline.run_batches: several batches in flight (record slots reused) on offset float32 tensors, pure columns included."""
    from quantization_analysis_amd.pipeline import GreedyPipeline

    batches = [np.stack([offset_tensor((128, 192), r, seed=50 + 3 * b + i) for i, r in enumerate((10.0, 1e3))]) for b in range(4)]
    with GreedyPipeline(ALL, "pcc", 0.999, 123, chunk=2, pure_formats=ALL) as pipe:
        got = pipe.run_batches([dev(b, False) for b in batches])
    for b, res in zip(batches, got):
        for i, r in enumerate(res):
            pcc_ok(r.pcc, b[i], orc.apply_assignment(b[i], r.assignment), f"run_batches tensor {i}")
            for f in ALL:
                pcc_ok(r.pure[f][0], b[i], quantize_weight_values(b[i], f), f"run_batches tensor {i} pure {f}")


def test_sweep_rows_and_baselines(monkeypatch):
    """sweep.sweep_tensor on the hip backend: every column it reports (baselines and step rows) against the float64 Pearson of the
    oracle's reconstruction under the map it was computed for."""
    from quantization_analysis_amd import sweep
    from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer

    x = offset_tensor((256, 384), 100.0, seed=60)
    seen = []
    orig = sweep.columns_from_stats

    def spy(ts, amap):
        c = orig(ts, amap)
        seen.append((np.asarray(amap, dtype=np.int8).reshape(ts.tiles_h, ts.tiles_w).copy(), c["pcc"]))
        return c

    monkeypatch.setattr(sweep, "columns_from_stats", spy)
    rows, baselines, _thr = sweep.sweep_tensor(dev(x, False), ALL, "pcc", 0.0, 8, Quantizer("hip"))
    assert len(seen) >= len(ALL) + 1 and len(baselines) >= 1
    for a, pcc in seen:
        pcc_ok(pcc, x, orc.apply_assignment(x, a), "sweep column")
    reported = {p for _a, p in seen}
    assert all(r["pcc"] in reported for r in rows) and all(b["pcc"] in reported for b in baselines)


def _table(path) -> dict:
    """wq's table.txt → {tensor: {FORMAT or MIXED: printed pcc}}."""
    out, cur = {}, None
    for line in path.read_text().splitlines():
        if line and not line.startswith(" "):
            cur = out.setdefault(line.strip(), {})
        elif cur is not None and (line.startswith("  none") or line.startswith("  mixed")):
            parts = line.split()
            cur[parts[1]] = float(parts[2])
    return out


def _wq(args, tmp_path):
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "wq"), *args, "--backend", "hip", "--no-plots", "--results-dir", str(tmp_path / "res")],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tables = list((tmp_path / "res").rglob("table.txt"))
    assert len(tables) == 1
    return _table(tables[0])


def test_wq_gpt2_ln_1(tmp_path):
    """`wq --backend hip synthetic:gpt2 h.0.ln_1.weight` (float32 ones + 0.01·N): every printed PCC within 1e-5 of the float64 Pearson."""
    import json

    from quantization_analysis_amd import model_source as ms

    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"algorithm": "mixed-tile-greedy", "seed": 123, "quantization_formats": ALL + PROXIES,
                               "params": {"metric": "pcc", "threshold": 0.999}}))
    table = _wq(["synthetic:gpt2", "h.0.ln_1.weight", "--compression-config", str(cfg)], tmp_path)
    x = ms.build_model_index("synthetic:gpt2").load("h.0.ln_1.weight").numpy()
    rows = table["h.0.ln_1.weight"]
    for f in ALL + PROXIES:
        want = orc.pearson_corr_f64(x, quantize_weight_values(x, f))
        assert abs(rows[f.upper()] - want) <= 1e-5, (f, rows[f.upper()], want)
    want = orc.pearson_corr_f64(x, reference_columns(x, orc.greedy(x, ALL, "pcc", 0.999, 123)[0].reshape(-1))[3])
    assert abs(rows["MIXED"] - want) <= 1e-5, (rows["MIXED"], want)


def test_wq_streamed_offset_model(tmp_path):
    """`wq --backend hip` with a search on a local model of offset float32 matrices: the streamed driver (a shape group of two, the
    none rows out of the search's records, the proxies over the resident (2, rows, cols) batch) and a vector on the per-tensor path."""
    import json

    from safetensors.torch import save_file

    rng = np.random.default_rng(70)
    mats = {"a.weight": (2.0 + 0.002 * rng.standard_normal((96, 160))).astype(np.float32),
            "b.weight": (-5.0 + 0.01 * rng.standard_normal((96, 160))).astype(np.float32),
            "n.weight": (1.0 + 0.001 * rng.standard_normal(300)).astype(np.float32)}
    (tmp_path / "model").mkdir()
    save_file({k: torch.from_numpy(v) for k, v in mats.items()}, str(tmp_path / "model" / "model.safetensors"))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"algorithm": "mixed-tile-greedy", "seed": 123, "quantization_formats": ALL + PROXIES,
                               "params": {"metric": "pcc", "threshold": 0.99}}))
    table = _wq([str(tmp_path / "model"), "--compression-config", str(cfg)], tmp_path)
    for name, x in mats.items():
        rows = table[name]
        for f in ALL + PROXIES:
            want = orc.pearson_corr_f64(x, reference_columns(x, np.full(_tiles(x), MIXED_TILE_FORMATS.index(f)))[3]
                                        if f in MIXED_TILE_FORMATS else quantize_weight_values(x, f))
            assert abs(rows[f.upper()] - want) <= 1e-5, (name, f, rows[f.upper()], want)
        a = orc.greedy(x, ALL, "pcc", 0.99, 123)[0]
        want = orc.pearson_corr_f64(x, reference_columns(x, a.reshape(-1))[3])
        assert abs(rows["MIXED"] - want) <= 1e-5, (name, rows["MIXED"], want)
