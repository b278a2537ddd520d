"""GPU: the mixed-tile searches over the transposed layout on the hip backend — K3T (mtq_apply_assignment_transposed) and the
transposed knife-edge gather (mtq_knife_tiles_transposed) against their row-layout kernels on a contiguous Xᵀ, the three algorithms
against the reference's results on np.transpose(x) (F16) and the emulation backend, and `wq --backend hip` with the example config."""
import hashlib
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms import create_algorithm
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from tests.inputs import gen
from tests.test_cli import strip_time

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
CONFIG = ROOT / "compression_configs" / "compression_config.mixed_tile_greedy_transpose.example.json"
ROWS_CONFIG = ROOT / "compression_configs" / "greedy_seed123.json"


@pytest.fixture(scope="module")
def f16():
    g = ROOT / "tests" / "golden"
    return np.load(g / "f16_mixed_transpose.npz"), json.loads((g / "golden_meta_f16.json").read_text())


def _torch():
    import torch

    hb.require_gpu()
    return torch


def _bits(y):
    y = y.cpu().numpy() if hasattr(y, "cpu") else y
    return np.ascontiguousarray(np.asarray(y, dtype=np.float32)).view(np.uint32)


def _inputs():
    specials = lambda: np.load(ROOT / "tests" / "golden" / "f16_mixed_transpose.npz")["specials__x"]   # noqa: E731  (F15's specials)
    rng = np.random.default_rng(316)
    out = [("s100x150", (rng.standard_normal((100, 150)) * 0.02).astype(np.float32)),
           ("s33x47", (rng.standard_normal((33, 47)) * np.exp(rng.standard_normal((33, 47)))).astype(np.float32)),
           ("s1x40", (rng.standard_normal((1, 40)) * 0.1).astype(np.float32)),
           ("s64x96", (rng.standard_normal((64, 96)) * 0.02).astype(np.float32)),
           ("s37x212", (rng.standard_normal((37, 212)) * np.exp(rng.standard_normal((37, 1)))).astype(np.float32)),
           ("specials", specials())]
    return out


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_k3t_equals_k3_on_a_contiguous_transpose(dtype):
    torch = _torch()
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(17)
    for name, x in _inputs():
        xd = torch.from_numpy(x).cuda().to(tdt)
        th, tw = hb.tiles_hw(x.shape[1], x.shape[0])
        amap = rng.integers(0, 4, size=(th, tw)).astype(np.int8)
        amap.reshape(-1)[: min(4, amap.size)] = np.arange(min(4, amap.size))           # every format code in one map
        want = hb.apply_assignment(xd.t().contiguous(), amap).t().contiguous()
        got = hb.apply_assignment_transposed(xd, amap)
        assert got.shape == xd.shape and got.dtype == torch.float32
        assert np.array_equal(_bits(got), _bits(want)), (name, dtype)
    # a batch: count > 1, one map per matrix, and a row-strided view read in place
    xb = torch.from_numpy((rng.standard_normal((3, 70, 90)) * 0.02).astype(np.float32)).cuda().to(tdt)
    th, tw = hb.tiles_hw(90, 70)
    maps = rng.integers(0, 4, size=(3, th * tw)).astype(np.int8)
    got = hb.apply_assignment_transposed(xb, maps)
    for i in range(3):
        want = hb.apply_assignment(xb[i].t().contiguous(), maps[i].reshape(th, tw)).t()
        assert np.array_equal(_bits(got[i]), _bits(want)), i
    wide = torch.from_numpy((rng.standard_normal((50, 160)) * 0.02).astype(np.float32)).cuda().to(tdt)
    view = wide[:, 16:16 + 100]
    th, tw = hb.tiles_hw(100, 50)
    amap = rng.integers(0, 4, size=(th, tw)).astype(np.int8)
    assert np.array_equal(_bits(hb.apply_assignment_transposed(view, amap)), _bits(hb.apply_assignment(view.t().contiguous(), amap).t()))
    # a batch whose columns are a multiple of 4: the vector form of K3T, with its per-matrix x, y and map offsets
    xq = torch.from_numpy((rng.standard_normal((3, 70, 100)) * np.exp(rng.standard_normal((3, 70, 1)))).astype(np.float32)).cuda().to(tdt)
    th, tw = hb.tiles_hw(100, 70)
    maps = rng.integers(0, 4, size=(3, th * tw)).astype(np.int8)
    got = hb.apply_assignment_transposed(xq, maps)
    for i in range(3):
        want = hb.apply_assignment(xq[i].t().contiguous(), maps[i].reshape(th, tw)).t()
        assert np.array_equal(_bits(got[i]), _bits(want)), ("quad batch", i)
    with pytest.raises(hb.MtqError, match="entries"):
        hb.apply_assignment_transposed(xb[0], np.zeros(int(np.prod(hb.tiles_hw(90, 70))) + 1, dtype=np.int8))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_transposed_knife_gather_equals_the_row_gather(dtype):
    torch = _torch()
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(18)
    fmts = ["bf16", "bfp8", "bfp4", "bfp2"]
    for name, x in _inputs() + [("batch", (rng.standard_normal((2, 72, 100)) * 0.02).astype(np.float32))]:
        x3 = torch.from_numpy(x if x.ndim == 3 else x[None]).cuda().to(tdt)
        count, rows, cols = x3.shape
        xt3 = torch.empty((count, cols, rows), dtype=tdt, device="cuda").copy_(x3.transpose(1, 2))   # fresh strides, also for 1-wide shapes
        tiles = count * int(np.prod(hb.tiles_hw(cols, rows)))
        near = torch.from_numpy((rng.random(tiles) < 0.5).astype(np.int8)).cuda()
        k = int(near.sum())
        outs = []
        for src, transposed in ((x3, True), (xt3, False)):
            lst = torch.empty((k + 1,), dtype=torch.int64, device="cuda")
            out = torch.empty((1 + len(fmts), k, 32, 32), dtype=torch.float32, device="cuda")
            hb.knife_tiles_device(src, near, fmts, k, lst, out, transposed=transposed)
            ids = lst[:k].cpu().numpy()
            assert int(lst[k]) == k
            order = np.argsort(ids)
            outs.append((ids[order], _bits(out)[:, order]))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), (name, dtype)


def _run(x, run, backend, tmp_path, layout="transpose"):
    with np.errstate(all="ignore"):
        res = create_algorithm(run["algorithm"], {**run["params"], "layout": layout}).run(
            x, FORMATS, Quantizer(backend), CacheContext(tmp_path, "t", backend, True, "gpu"))
    return res[0]


def test_hip_algorithms_match_f16_and_emulation(f16, tmp_path):
    torch = _torch()
    data, meta = f16
    for run in meta["runs"]:
        x = data[f"{run['case']}__x"]
        name = run["run"]
        r = _run(x, run, "hip", tmp_path)                                        # host input: host output
        assert r.compression == run["algorithm"] + "+transpose", name
        assert np.array_equal(r.meta["assignment"], data[f"{name}__map"]), name
        assert [r.tile_counts[f] for f in MIXED_TILE_FORMATS] == run["counts"] and r.tile_bytes == run["tile_bytes"], name
        assert isinstance(r.y, np.ndarray) and np.array_equal(_bits(r.y), data[f"{name}__y"]), name
        e = _run(x, run, "emulation", tmp_path)
        assert np.array_equal(e.meta["assignment"], r.meta["assignment"]) and e.tile_counts == r.tile_counts, name
        d = _run(torch.from_numpy(x).cuda(), run, "hip", tmp_path)               # device input: device output
        assert d.y.is_cuda and np.array_equal(_bits(d.y), data[f"{name}__y"]), name
        assert np.array_equal(d.meta["assignment"], data[f"{name}__map"]), name
    # bf16 storage: the bf16-valued case read as bfloat16
    for run in [r for r in meta["runs"] if r["case"] == "s96x160"]:
        xb = torch.from_numpy(data["s96x160__x"]).cuda().to(torch.bfloat16)
        r = _run(xb, run, "hip", tmp_path)
        assert np.array_equal(r.meta["assignment"], data[f"{run['run']}__map"]) and np.array_equal(_bits(r.y), data[f"{run['run']}__y"]), run["run"]


def test_hip_algorithms_match_f16_large(f16, tmp_path):
    torch = _torch()
    _, meta = f16
    big = meta["big"]
    x = gen(big["kind"], big["seed"], tuple(big["shape"]))
    xb = torch.from_numpy(x).cuda().to(torch.bfloat16)                           # bf16-valued: the weight as a checkpoint stores it
    for run in big["runs"]:
        r = _run(xb, run, "hip", tmp_path)
        amap = np.ascontiguousarray(r.meta["assignment"], dtype=np.int8)
        assert hashlib.sha256(amap.tobytes()).hexdigest() == run["map_sha256"], run["run"]
        assert [r.tile_counts[f] for f in MIXED_TILE_FORMATS] == run["counts"], run["run"]
        assert hashlib.sha256(np.ascontiguousarray(r.y.cpu().numpy()).tobytes()).hexdigest() == run["y_sha256"], run["run"]


def test_knife_edge_and_rank_three_routes(f16, tmp_path):
    """Knife-edge thresholds gather Xᵀ tiles in place (rank 2); a rank-3 tensor takes the permuted copy."""
    from quantization_analysis_amd.compression_algorithms import tile_search

    torch = _torch()
    data, meta = f16
    knife = [r for r in meta["runs"] if r["case"] == "s100x150" and "knife" in r["run"]]
    assert knife
    for run in knife:
        r = _run(data["s100x150__x"], run, "hip", tmp_path)
        assert r.meta["knife_edge_tiles"] >= 1, run["run"]
        assert np.array_equal(r.meta["assignment"], data[f"{run['run']}__map"]), run["run"]
    x3 = torch.from_numpy(data["s3x40x72__x"]).cuda()
    ts = tile_search.compute_tile_stats(x3, ["bfp8", "bfp4"], Quantizer("hip"), layout="transpose")
    assert not ts.transposed and (ts.tiles_h, ts.tiles_w) == (90, 1)
    ts2 = tile_search.compute_tile_stats(x3[0], ["bfp8", "bfp4"], Quantizer("hip"), layout="transpose")
    assert ts2.transposed and ts2.x2d.data_ptr() == x3[0].data_ptr()           # rank 2: read in place, no transposed copy
    ref = tile_search.compute_tile_stats(x3[0].t().contiguous(), ["bfp8", "bfp4"], Quantizer("hip"))
    assert np.array_equal(ts2.stats, ref.stats, equal_nan=True)


def _wq(tmp_path, backend, config, *extra):
    out_dir = tmp_path / f"{backend}{''.join(extra)}{config.stem}"
    out = subprocess.run([sys.executable, str(ROOT / "wq"), "synthetic:tiny", "--backend", backend, "--compression-config", str(config),
                          "--results-dir", str(out_dir), "--no-plots", *extra], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    return out.stdout, out_dir


def _rows(text, comp):
    return [ln.split() for ln in text.splitlines() if ln.startswith(f"  {comp} ")]


def _table(text):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("model."))
    end = next(i for i, ln in enumerate(lines) if ln.startswith("results:"))
    return strip_time("\n".join(lines[start:end]))


def _maps(out_dir):
    return {p.parent.name: np.load(p) for p in out_dir.glob("*/*/*/*/*/assignment.npy")}


def test_wq_hip_with_the_example_config(tmp_path):
    emu, emu_dir = _wq(tmp_path, "emulation", CONFIG)
    lit, _ = _wq(tmp_path, "hip", CONFIG, "--literal-metrics")
    assert _table(lit) == _table(emu)
    fast, fast_dir = _wq(tmp_path, "hip", CONFIG)
    assert re.search(r"streamed [1-9]\d* tensors in", fast)                   # the 2-D tensors through GreedyPipeline(layout="transpose")
    me, mf = _maps(emu_dir), _maps(fast_dir)
    assert me and me.keys() == mf.keys() and all(np.array_equal(me[k], mf[k]) for k in me)
    slow, slow_dir = _wq(tmp_path, "hip", CONFIG, "--no-stream")               # the per-tensor route: the same maps and counts
    ms_ = _maps(slow_dir)
    assert ms_.keys() == mf.keys() and all(np.array_equal(ms_[k], mf[k]) for k in ms_)
    assert [r[7:] for r in _rows(slow, "mixed-tile-greedy+transpose")] == [r[7:] for r in _rows(fast, "mixed-tile-greedy+transpose")]
    re_, rf = _rows(emu, "mixed-tile-greedy+transpose"), _rows(fast, "mixed-tile-greedy+transpose")
    assert len(re_) == len(rf) > 0
    for a, b in zip(re_, rf):
        assert a[7:] == b[7:]                                                    # tile counts and bytes
        assert abs(float(a[2]) - float(b[2])) <= 2e-4
        assert np.allclose([float(v) for v in a[3:5]], [float(v) for v in b[3:5]], rtol=2e-3, atol=0)
    # the `none` rows of a transposed run are those of a row-layout run of the same tensors
    rows_run, _ = _wq(tmp_path, "hip", ROWS_CONFIG)
    nt, nr = _rows(fast, "none"), _rows(rows_run, "none")
    assert len(nt) == len(nr) > 0
    for a, b in zip(nt, nr):
        assert a[:5] + a[6:] == b[:5] + b[6:]                                    # the printed text, TIME(s) aside
        assert all(abs(float(u) - float(v)) <= 1e-12 for u, v in zip(a[2:5], b[2:5]))


MIXED = ["bf16", "bfp8", "bfp4", "bfp2"]


def _batches(torch):
    """Two shape groups of three tensors: bf16 storage (96x160, the identity bf16 records) and float32 storage (70x130, ragged)."""
    a = np.stack([gen("normal_bf16", 160 + i, (96, 160)) for i in range(3)])
    b = np.stack([gen("heavy_f32", 170 + i, (70, 130)) for i in range(3)])
    return [(a, torch.from_numpy(a).cuda().to(torch.bfloat16)), (b, torch.from_numpy(b).cuda())]


def _per_tensor(x, alg, params, tmp_path):
    return _run(x, {"algorithm": alg, "params": params}, "hip", tmp_path)


@pytest.mark.parametrize("scan", ["device", "host"])
def test_greedy_pipeline_transpose_equals_per_tensor(scan, tmp_path):
    from oracle import mtq_oracle as orc
    from quantization_analysis_amd.pipeline import GreedyPipeline

    torch = _torch()
    groups = _batches(torch)
    params = {"metric": "pcc", "threshold": 0.998, "seed": 123}
    with GreedyPipeline(MIXED, "pcc", 0.998, 123, chunk=2, workers=2, scan=scan, layout="transpose") as pipe:
        assert pipe.device_scan == (scan == "device") and pipe.lazy_plan(groups[0][1]) is None
        single = [pipe.run(xd) for _x, xd in groups]
        batched = pipe.run_batches([xd for _x, xd in groups])
    for (x, xd), res, res_b in zip(groups, single, batched):
        assert len(res) == len(res_b) == 3
        for j, (r, rb) in enumerate(zip(res, res_b)):
            want = _per_tensor(np.asarray(xd[j].float().cpu()), "mixed-tile-greedy", params, tmp_path)
            assert r.assignment.shape == want.meta["assignment"].shape == hb.tiles_hw(x.shape[2], x.shape[1])
            assert np.array_equal(r.assignment, want.meta["assignment"]) and r.counts == want.tile_counts, (x.shape, j)
            assert np.array_equal(rb.assignment, r.assignment) and rb.counts == r.counts
            a, counts, _st = orc.greedy(np.ascontiguousarray(np.asarray(xd[j].float().cpu()).T), MIXED, "pcc", 0.998, 123)
            assert np.array_equal(r.assignment, a) and r.counts == counts
            c = want.meta["columns"]
            assert abs(r.pcc - c["pcc"]) <= 1e-12 and abs(r.mae - c["mae"]) <= 1e-12 * c["mae"] and r.atol == c["atol"], (x.shape, j)


@pytest.mark.parametrize("scan", ["device", "host"])
def test_greedy_pipeline_transpose_hand_back(scan, tmp_path):
    """A zero-variance tensor in a device-scanned batch is handed back to the host scan, on its records recomputed by K1T."""
    from quantization_analysis_amd.pipeline import GreedyPipeline

    torch = _torch()
    xs = np.stack([gen("normal_bf16", 190, (64, 96)), np.full((64, 96), 0.5, dtype=np.float32), gen("normal_bf16", 191, (64, 96))])
    xd = torch.from_numpy(xs).cuda().to(torch.bfloat16)
    with GreedyPipeline(MIXED, "pcc", 0.998, 123, chunk=3, workers=2, scan=scan, layout="transpose") as pipe:
        res = pipe.run(xd)
    assert pipe.host_fallbacks == (1 if scan == "device" else 0)
    for j, r in enumerate(res):
        want = _per_tensor(xs[j], "mixed-tile-greedy", {"metric": "pcc", "threshold": 0.998, "seed": 123}, tmp_path)
        assert np.array_equal(r.assignment, want.meta["assignment"]) and r.counts == want.tile_counts, j


@pytest.mark.parametrize("cap", [128, 1])
@pytest.mark.parametrize("chunk", [16, 1])
def test_threshold_pipeline_transpose_equals_per_tensor(f16, cap, chunk, tmp_path):
    """ThresholdPipeline in transpose mode (one chunk: mtq_threshold_enqueue_transposed; several: K1T + the transposed gather call by call),
    at a knife-edge threshold, knife_cap 1 included (more knife-edge tiles than the list holds: the indexed gather of Xᵀ tiles)."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    torch = _torch()
    data, meta = f16
    run = next(r for r in meta["runs"] if r["run"] == "s100x150__thr_pcc_knife_eq")
    thr = run["params"]["threshold"]
    rng = np.random.default_rng(5)
    xs = np.stack([data["s100x150__x"]] + [(rng.standard_normal((100, 150)) * 0.02).astype(np.float32) for _ in range(2)])
    ys = np.stack([data["s100x150__x"]] * 3)          # three knife-edge tiles in one chunk: more than knife_cap 1 lists
    knife_total = 0
    for batch in (xs, ys):
        xd = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
        with ThresholdPipeline(MIXED, "pcc", thr, chunk=chunk, layout="transpose") as pipe:
            pipe.knife_cap = cap
            res = pipe.run(xd)
            res_b = pipe.run_batches([xd])[0]
            knife_total += pipe.knife_tiles
        for j, (r, rb) in enumerate(zip(res, res_b)):
            want = _per_tensor(batch[j], "mixed-tile-threshold", {"metric": "pcc", "threshold": thr}, tmp_path)
            assert np.array_equal(r.assignment, want.meta["assignment"]) and r.counts == want.tile_counts, (cap, chunk, j)
            assert np.array_equal(rb.assignment, r.assignment)
            c = want.meta["columns"]
            assert abs(r.pcc - c["pcc"]) <= 1e-12 and abs(r.mae - c["mae"]) <= 1e-12 * c["mae"] and r.atol == c["atol"]
    assert np.array_equal(res[0].assignment, data["s100x150__thr_pcc_knife_eq__map"]) and knife_total >= 3


def test_reconstruct_script_on_hip(tmp_path):
    """scripts/reconstruct_mixed_tile_assignment.py --layout transpose on hip (K3T for a 2-D tensor, the permuted copy through K3 for a
    rank-3 one) gives the emulation backend's y."""
    import torch
    from safetensors.torch import save_file

    _torch()
    rng = np.random.default_rng(23)
    model = tmp_path / "model"
    model.mkdir()
    tensors = {"w2": torch.from_numpy((rng.standard_normal((70, 100)) * 0.02).astype(np.float32)).to(torch.bfloat16),
               "w3": torch.from_numpy((rng.standard_normal((3, 40, 72)) * 0.02).astype(np.float32))}
    save_file(tensors, str(model / "model.safetensors"))
    script = ROOT / "scripts" / "reconstruct_mixed_tile_assignment.py"
    for name, t in tensors.items():
        x = t.float().numpy()
        xt = np.transpose(x)
        grid = (-(-xt.reshape(-1, xt.shape[-1]).shape[0] // 32), -(-xt.shape[-1] // 32))
        amap = rng.integers(0, 4, size=grid).astype(np.int8)
        np.save(tmp_path / f"{name}_a.npy", amap)
        ys = {}
        for backend in ("emulation", "hip"):
            out = subprocess.run([sys.executable, str(script), str(model), name, str(tmp_path / f"{name}_a.npy"), "--layout", "transpose",
                                  "--backend", backend, "--out", str(tmp_path / f"{name}_{backend}.npy")], cwd=tmp_path, capture_output=True,
                                 text=True, timeout=600)
            assert out.returncode == 0, out.stdout + out.stderr
            ys[backend] = np.load(tmp_path / f"{name}_{backend}.npy")
        assert ys["hip"].shape == x.shape and np.array_equal(_bits(ys["hip"]), _bits(ys["emulation"])), name
