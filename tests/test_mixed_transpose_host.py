"""CPU-only: the mixed-tile searches over the transposed layout (params["layout"] = "transpose") — the emulation results against the
reference's on np.transpose(x) (F16), the `layout` check, the row layout left as it was, rank <= 1 and rank >= 3, `wq` with the example
config, and the reconstruct script with --layout transpose."""
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from quantization_analysis_amd.cli import _columns_emulation
from quantization_analysis_amd.compression_algorithms import create_algorithm
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import compute_tile_stats
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from tests.inputs import gen

ROOT = Path(__file__).resolve().parent.parent
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
ALGOS = ["mixed-tile-greedy", "mixed-tile", "mixed-tile-threshold", "mixed-tile-random"]
CONFIG = ROOT / "compression_configs" / "compression_config.mixed_tile_greedy_transpose.example.json"


@pytest.fixture(scope="module")
def f16(golden_dir):
    return np.load(golden_dir / "f16_mixed_transpose.npz"), json.loads((golden_dir / "golden_meta_f16.json").read_text())


def _cache(tmp_path):
    return CacheContext(root=tmp_path, tensor_name="t", backend="emulation", recompute=True, run_tag="test")


def _run(x, alg, params, tmp_path, backend="emulation"):
    with np.errstate(all="ignore"):
        res = create_algorithm(alg, params).run(x, FORMATS, Quantizer(backend), _cache(tmp_path))
    assert len(res) == 1
    return res[0]


def _bits(y):
    return np.ascontiguousarray(np.asarray(y, dtype=np.float32)).view(np.uint32)


def test_emulation_reproduces_f16(f16, tmp_path):
    data, meta = f16
    assert len(meta["runs"]) >= 40
    for run in meta["runs"]:
        x = data[f"{run['case']}__x"]
        r = _run(x, run["algorithm"], {**run["params"], "layout": "transpose"}, tmp_path)
        name = run["run"]
        assert r.compression == run["algorithm"] + "+transpose", name
        assert np.array_equal(r.meta["assignment"], data[f"{name}__map"]), name
        assert [r.tile_counts[f] for f in MIXED_TILE_FORMATS] == run["counts"], name
        assert r.tile_bytes == run["tile_bytes"], name
        assert np.array_equal(_bits(r.y), data[f"{name}__y"]), name
        with np.errstate(all="ignore"):
            cols = _columns_emulation(x, np.asarray(r.y, dtype=np.float32))
        for k, v in zip(("pcc", "mae", "atol"), cols):
            assert np.array_equal(np.float32(v), np.float32(run[k]), equal_nan=True), (name, k)


def test_emulation_reproduces_f16_large(f16, tmp_path):
    _, meta = f16
    big = meta["big"]
    x = gen(big["kind"], big["seed"], tuple(big["shape"]))
    assert hashlib.sha256(x.tobytes()).hexdigest() == big["x_sha256"]
    for run in big["runs"]:
        r = _run(x, run["algorithm"], {**run["params"], "layout": "transpose"}, tmp_path)
        amap = np.ascontiguousarray(r.meta["assignment"], dtype=np.int8)
        assert list(amap.shape) == run["map_shape"] == [128, 32], run["run"]
        assert hashlib.sha256(amap.tobytes()).hexdigest() == run["map_sha256"], run["run"]
        assert [r.tile_counts[f] for f in MIXED_TILE_FORMATS] == run["counts"], run["run"]
        assert hashlib.sha256(np.ascontiguousarray(r.y, dtype=np.float32).tobytes()).hexdigest() == run["y_sha256"], run["run"]


@pytest.mark.parametrize("alg", ALGOS)
def test_layout_is_validated(alg):
    for bad in ("cols", "TRANSPOSE", "", None, 1):
        with pytest.raises(ValueError, match="layout"):
            create_algorithm(alg, {"layout": bad})
    assert create_algorithm(alg, {}).layout == "rows"
    assert create_algorithm(alg, {"layout": "rows"}).layout == "rows"
    assert create_algorithm(alg, {"layout": "transpose"}).layout == "transpose"
    with pytest.raises(ValueError, match="layout"):
        compute_tile_stats(np.zeros((4, 4), dtype=np.float32), ["bfp8"], Quantizer("emulation"), layout="cols")


@pytest.mark.parametrize("alg", ALGOS)
def test_rows_and_absent_layout_are_todays_results(alg, tmp_path):
    x = (np.random.default_rng(11).standard_normal((70, 100)) * 0.02).astype(np.float32)
    params = {"threshold": 0.995, "seed": 4, "iters": 6}
    a = _run(x, alg, params, tmp_path)
    b = _run(x, alg, {**params, "layout": "rows"}, tmp_path)
    t = _run(x, alg, {**params, "layout": "transpose"}, tmp_path)
    assert a.compression == b.compression == create_algorithm(alg).name
    assert a.meta["assignment"].shape == (3, 4) and np.array_equal(a.meta["assignment"], b.meta["assignment"])
    assert a.tile_counts == b.tile_counts and np.array_equal(_bits(a.y), _bits(b.y))
    assert t.compression == a.compression + "+transpose" and t.meta["assignment"].shape == (4, 3)


@pytest.mark.parametrize("alg", ALGOS)
@pytest.mark.parametrize("shape", [(1003,), (), (1, 40)])
def test_rank_at_most_one_equals_rows(alg, shape, tmp_path):
    """np.transpose is the identity below rank 2: the transposed run is the row-layout run, maps included.  (1, 40) is rank 2: its
    transpose (40, 1) has a grid of its own."""
    x = (np.random.default_rng(12).standard_normal(shape) * 0.1).astype(np.float32)
    params = {"threshold": 0.99, "seed": 2, "iters": 5}
    rows = _run(x, alg, params, tmp_path)
    t = _run(x, alg, {**params, "layout": "transpose"}, tmp_path)
    assert t.compression == rows.compression + "+transpose"
    assert np.asarray(t.y).shape == x.shape
    if len(shape) <= 1:
        assert np.array_equal(t.meta["assignment"], rows.meta["assignment"]) and t.tile_counts == rows.tile_counts
        assert np.array_equal(_bits(t.y), _bits(rows.y))
    else:
        ref = _run(np.ascontiguousarray(x.T), alg, params, tmp_path)
        assert np.array_equal(t.meta["assignment"], ref.meta["assignment"])
        assert np.array_equal(_bits(t.y), _bits(np.ascontiguousarray(np.asarray(ref.y).T)))


def test_rank_three_reverses_every_axis(f16, tmp_path):
    """np.transpose of a rank-3 tensor reverses all axes: its 2-D view is not V.T for V = x.reshape(d0, -1), and neither are its tiles.
    The golden maps are those of the reversed tensor; the V.T route gives other maps."""
    data, meta = f16
    x = data["s3x40x72__x"]
    runs = [r for r in meta["runs"] if r["case"] == "s3x40x72"]
    assert runs
    v_t = np.ascontiguousarray(x.reshape(x.shape[0], -1).T)
    rev = np.ascontiguousarray(np.transpose(x)).reshape(-1, x.shape[0])
    assert v_t.shape == rev.shape and not np.array_equal(v_t, rev)
    differs = 0
    for run in runs:
        via_v = _run(v_t, run["algorithm"], run["params"], tmp_path)
        differs += not np.array_equal(_bits(np.asarray(via_v.y).T.reshape(x.shape)), data[f"{run['run']}__y"])
    assert differs > 0
    ts = compute_tile_stats(x, ["bfp8", "bfp2"], Quantizer("emulation"), layout="transpose")
    ref = compute_tile_stats(np.transpose(x), ["bfp8", "bfp2"], Quantizer("emulation"))
    assert (ts.tiles_h, ts.tiles_w) == (ref.tiles_h, ref.tiles_w) == (72 * 40 // 32, 1)
    assert np.array_equal(ts.stats, ref.stats, equal_nan=True)


def test_wq_emulation_prints_transpose_rows(tmp_path):
    out = subprocess.run([sys.executable, str(ROOT / "wq"), "synthetic:tiny", "--backend", "emulation", "--limit", "2",
                          "--compression-config", str(CONFIG), "--results-dir", str(tmp_path), "--no-plots", "--summary"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert "compression: none, mixed-tile-greedy+transpose" in lines
    mixed = [ln for ln in lines if ln.startswith("  mixed-tile-greedy+transpose ")]
    assert len(mixed) >= 3 and all(ln.split()[1] == "MIXED" for ln in mixed)        # table rows and the summary row
    assert not any(ln.startswith("  mixed-tile-greedy ") for ln in lines)
    run_dirs = list(tmp_path.glob("synthetic__tiny/mixed-tile-greedy+transpose/*"))
    assert len(run_dirs) == 1
    used = json.loads((run_dirs[0] / "compression_config.used.json").read_text())
    assert used["algorithm"] == "mixed-tile-greedy" and used["params"]["layout"] == "transpose" and used["seed"] == 123
    maps = sorted(run_dirs[0].glob("mixed_tile_greedy+transpose/*/assignment.npy"))
    assert maps
    for p in maps:
        shape = json.loads((p.parent / "assignment_mapping.json").read_text())["assignment_shape"]
        assert list(np.load(p).shape) == shape


def test_reconstruct_script_with_transposed_map(tmp_path):
    """The script rebuilds the search's y from the map wq wrote for the transposed grid."""
    from quantization_analysis_amd.model_source import build_model_index

    index = build_model_index("synthetic:tiny")
    name = next(n for n in sorted(index.specs) if len(index.specs[n].shape) == 2 and min(index.specs[n].shape) > 32
                and index.specs[n].shape[0] != index.specs[n].shape[1])
    x = np.asarray(index.load(name).float().numpy(), dtype=np.float32)
    r = _run(x, "mixed-tile-greedy", {"threshold": 0.999, "seed": 123, "layout": "transpose"}, tmp_path)
    amap = r.meta["assignment"]
    assert amap.shape == (-(-x.shape[1] // 32), -(-x.shape[0] // 32))
    np.save(tmp_path / "a.npy", amap)
    script = ROOT / "scripts" / "reconstruct_mixed_tile_assignment.py"
    out = subprocess.run([sys.executable, str(script), "synthetic:tiny", name, str(tmp_path / "a.npy"), "--layout", "transpose",
                          "--out", str(tmp_path / "y.npy")], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(_bits(np.load(tmp_path / "y.npy")), _bits(r.y))
    wrong = subprocess.run([sys.executable, str(script), "synthetic:tiny", name, str(tmp_path / "a.npy"), "--out", str(tmp_path / "z.npy")],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert wrong.returncode == 0                                              # as many tiles, read as the row grid: another y
    assert not np.array_equal(_bits(np.load(tmp_path / "z.npy")), _bits(r.y))


def test_wq_random_transpose_keeps_its_sample_outputs(tmp_path):
    """mixed-tile-random over the transposed layout writes the per-sample CSV and map under mixed_tile_random/, as the row layout does."""
    cfg = tmp_path / "random_t.json"
    cfg.write_text(json.dumps({"algorithm": "mixed-tile-random", "quantization_formats": FORMATS,
                               "params": {"metric": "pcc", "threshold": 0.99, "iters": 4, "seed": 3, "layout": "transpose"}}))
    out = subprocess.run([sys.executable, str(ROOT / "wq"), "synthetic:tiny", "model.layers.0.attn.k.weight", "--backend", "emulation",
                          "--compression-config", str(cfg), "--results-dir", str(tmp_path / "r"), "--no-plots"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    run_dir = next((tmp_path / "r").glob("synthetic__tiny/mixed-tile-random+transpose/*"))
    csvs = list(run_dir.glob("mixed_tile_random/*.csv"))
    maps = list(run_dir.glob("mixed_tile_random/*_assignment.npy"))
    assert len(csvs) == 1 and len(maps) == 1 and len(csvs[0].read_text().splitlines()) == 5   # header + 4 samples
    assert np.load(maps[0]).shape == (3, 2)                                              # Xᵀ of a 50x70 tensor: 3 x 2 tiles
    assert not list(run_dir.glob("mixed_tile_random+transpose"))
