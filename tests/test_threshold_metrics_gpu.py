"""The threshold search's device routes under mae and atol, end to end, on the inputs of tests/test_threshold_metrics_host.py (which
checks on the CPU what is relied on here: every knife threshold puts tiles inside the band and splits the map over formats, the
2^-60 input is knife-edge on every tile, the 2^20 / 2^40 thresholds lie above 1): ThresholdPipeline.run in several chunks (K1 →
threshold_assign_device_raw → knife_tiles_device call by call) and in one (mtq_threshold_enqueue), with the knife-edge list at its
default length, at 1 and at 0 (the extra trip); run_batches with ragged groups on and off; layout="transpose"; the reference's
fixtures; the `hip` plugin; the sweep script and wq.  Every map is the literal float32 rule's (orc.threshold); the columns are those of
the oracle's reconstruction.  (K4 on the device against K4 on the host for these metrics: tests/test_threshold_band_gpu.py.)"""
import csv
import json
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mtq_oracle as orc
from quantization_analysis_amd import cli, hip_backend as hb, model_source
from tests import test_threshold_metrics_host as tm
from tests.inputs import gen
from tests.test_cli import run_dir, write_cfg
from tests.test_golden_r2 import run_package_algo
from tests.test_threshold_band import bf16_values, knife_thresholds, oracle_maps, scaled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
DEFAULT_CAP = 128            # settings().knife_cap without MTQ_KNIFE_CAP
UNIT_SCALE = ("2^0", "heavy_f32", "heavy_bf16", "offset")   # the inputs whose pcc column is asserted (values of order 1e-2 .. 1)


def dev(x: np.ndarray, bf16: bool):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16).cuda() if bf16 else t.cuda()


def batch(label: str, n: int) -> np.ndarray:
    """n equally shaped tensors of a case: the case itself TWICE (a threshold ON one of its tiles' scores meets that score twice in the
    first chunk, more than a list of one entry holds), then the case at other seeds."""
    x0 = tm.make(label)
    return np.stack([x0, x0] + [tm.make(label, s) for s in range(1, n - 1)])


def all_knife_batch() -> np.ndarray:
    """N(0, 0.02²)·2^-60 at 256x512: 128 tiles a tensor, every one of them knife-edge at any threshold near its scores (the band is
    2e-6 absolute there) — two tensors of a chunk already overflow the default list of 128."""
    return np.stack([scaled(-60, seed=7900 + i, shape=(256, 512)) for i in range(3)])


BATCHES = [("2^-60", all_knife_batch, False), ("2^0", lambda: batch("2^0", 4), False), ("2^40", lambda: batch("2^40", 3), False),
           ("heavy_f32", lambda: batch("heavy_f32", 5), False), ("heavy_bf16", lambda: batch("heavy_bf16", 3), True),
           ("offset", lambda: batch("offset", 3), False)]


def spy_on_extra_trip(pipe) -> list:
    """Counts the indexed gathers of ThresholdPipeline.decide's "more knife-edge tiles than the list holds" branches (nothing else calls
    _knife_tiles_device)."""
    calls, inner = [], pipe._knife_tiles_device

    def counted(*args):
        calls.append(int(args[1].numel()))
        return inner(*args)

    pipe._knife_tiles_device = counted
    return calls


def same(r1, r2) -> bool:
    return (np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts
            and (r1.pcc, r1.mae, r1.atol, r1.metric_value) == (r2.pcc, r2.mae, r2.atol, r2.metric_value))


def check_columns(r, x: np.ndarray, a: np.ndarray, metric: str, pcc: bool, where) -> None:
    """The columns of a result against the oracle's reconstruction under map `a`.  atol: the exact float32 maximum.  mae: K1's |x − y|
    terms are exact float32 values summed in float64, so only the order of the sum differs from the reference's: numel·2^-53 relative
    to the exactly rounded float64 mean, at every scale.  pcc (unit-scale inputs): 1e-7 of the float64 two-pass Pearson."""
    with np.errstate(all="ignore"):
        y = orc.apply_assignment(x, a)
        d = np.abs(x.astype(np.float64) - y.astype(np.float64)).reshape(-1)
    assert r.atol == float(np.max(np.abs(x - y))), where
    assert r.metric_value == (r.mae if metric == "mae" else r.atol), where
    mean = math.fsum(d) / d.size
    assert abs(r.mae - mean) <= d.size * 2.0 ** -53 * mean, (where, r.mae, mean)
    if pcc:
        assert abs(r.pcc - orc.pearson_corr_f64(x, y)) <= 1e-7, (where, r.pcc)


@pytest.mark.parametrize("metric", ["mae", "atol"])
@pytest.mark.parametrize("label,make_batch,bf16", BATCHES, ids=[b[0] for b in BATCHES])
def test_pipeline_run_both_chunkings_every_list_length(label, make_batch, bf16, metric):
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    xs = make_batch()
    count, tiles = xs.shape[0], int(np.prod(hb.tiles_hw(*xs.shape[1:])))
    knife, far = tm.thresholds(xs[0], metric)
    wants = [oracle_maps(x, metric, knife + [far])[1] for x in xs]
    xd = dev(xs, bf16)
    for t, thr in enumerate(knife + [far]):
        for cap in (None, 1, 0):
            runs = []
            for chunk in (2, 8):                      # several chunks: the calls one by one; one chunk: mtq_threshold_enqueue
                pipe = ThresholdPipeline(ALL, metric, thr, chunk=chunk)
                if cap is not None:
                    pipe.knife_cap = cap
                trips = spy_on_extra_trip(pipe)
                with np.errstate(all="ignore"):
                    res = pipe.run(xd)
                where = (label, metric, thr, cap, chunk)
                assert [r.index for r in res] == list(range(count)), where
                for i, r in enumerate(res):
                    want = wants[i][t]
                    assert np.array_equal(r.assignment, want), (where, i, int(np.sum(r.assignment != want)))
                    assert r.counts == {f: int(np.sum(want == c)) for c, f in enumerate(ALL)}, (where, i)
                    check_columns(r, xs[i], want, metric, label in UNIT_SCALE, (where, i))
                if thr == far:
                    assert pipe.knife_tiles == 0 and not trips, where
                else:
                    assert pipe.knife_tiles > 0, where
                    if cap is not None:
                        assert pipe.knife_tiles > cap and trips, (where, pipe.knife_tiles)    # the extra trip really ran
                    if label == "2^-60":                  # every tile of every tensor: the default list overflows as well
                        assert pipe.knife_tiles == count * tiles and min(chunk, count) * tiles > DEFAULT_CAP and trips, (where, pipe.knife_tiles)
                pipe.close()
                runs.append(res)
            assert all(same(r1, r2) for r1, r2 in zip(*runs)), (label, metric, thr, cap)


def ragged_mix():
    """(host values the oracle takes, device batch, element count | None): vectors in their (ceil(n/32), 32) form, ragged and whole-tile
    matrices, both storage types (the 128x256 bf16 one takes the LDS-staged K1 and a launch chain of its own), and more float32 matrices
    than one ragged table holds.  The 96x160 matrix the thresholds are taken from is there twice (rows rolled by a tile): two matrices
    of the first ragged group own a knife-edge tile, more than a list of one entry holds."""
    hosts = [(tm.make("vector_1000"), False), (bf16_values(tm.make("vector")), True), (tm.make("ragged_33x17"), False), (tm.make("ragged_65x81"), False),
             (tm.make("heavy_f32"), False), (tm.make("2^0"), False), (np.roll(tm.make("2^0"), 32, axis=0), False), (tm.make("2^-60"), False), (tm.make("degenerate"), False), (tm.make("offset"), False),
             (tm.make("heavy_bf16"), True), (bf16_values(tm.make("ragged_65x81", 1)), True)]
    shapes = [(70, 100), (32, 32), (96, 160), (33, 17), (64, 200)]
    hosts += [(gen("heavy_f32" if i % 2 else "normal_f32", 7800 + i, shapes[i % len(shapes)]), False) for i in range(hb.RAGGED_MAX - 4)]
    out = []
    for h, bf16 in hosts:
        if h.ndim == 1:
            out.append((h, dev(tm.vector_form(h), bf16)[None], h.size))
        else:
            out.append((h, dev(h, bf16)[None], None))
    assert sum(1 for h, bf16 in hosts if not bf16) > hb.RAGGED_MAX                    # two ragged groups of float32 matrices
    return out


@pytest.mark.parametrize("knife_cap", [128, 1])
@pytest.mark.parametrize("metric", ["mae", "atol"])
def test_run_batches_ragged_switch_on_and_off(monkeypatch, metric, knife_cap):
    from quantization_analysis_amd.pipeline import ThresholdPipeline
    from quantization_analysis_amd.settings import settings

    mix = ragged_mix()
    knife, _far = tm.thresholds(tm.make("2^0"), metric)
    try:
        for thr in (knife[0], knife[3]):                 # ON a bfp8 and ON a bfp4 tile score of the 96x160 matrix
            runs = {}
            for ragged in ("1", "0"):
                monkeypatch.setenv("MTQ_THRESHOLD_RAGGED", ragged)
                monkeypatch.setenv("MTQ_KNIFE_CAP", str(knife_cap))
                settings(refresh=True)
                with ThresholdPipeline(ALL, metric, thr, chunk=2) as pipe:
                    trips = spy_on_extra_trip(pipe)
                    with np.errstate(all="ignore"):
                        runs[ragged] = pipe.run_batches([(x, n) for _h, x, n in mix])
                    assert pipe.knife_tiles > 0, (metric, thr, ragged)
                    if knife_cap == 1:
                        assert pipe.knife_tiles > 1, (metric, thr, ragged, pipe.knife_tiles)
                        if ragged == "1":                # the matrix-by-matrix trip: one gather per matrix that owns a knife-edge tile
                            assert len(trips) > 1, (metric, thr, trips)
            for i, (h, _x, _n) in enumerate(mix):
                r1, r0 = runs["1"][i][0], runs["0"][i][0]
                assert same(r1, r0) and r1.index == 0, (metric, thr, i)
                with np.errstate(all="ignore"):
                    a, counts, _sc = orc.threshold(h, ALL, metric, thr)
                assert np.array_equal(r1.assignment.reshape(-1), a.reshape(-1)) and r1.counts == counts, (metric, thr, i)
                check_columns(r1, h, a, metric, False, (metric, thr, i))
    finally:
        monkeypatch.undo()
        settings(refresh=True)


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("chunk", [16, 2])
@pytest.mark.parametrize("metric", ["mae", "atol"])
def test_transposed_layout(metric, chunk, cap):
    """layout="transpose" (one chunk: mtq_threshold_enqueue_transposed; several: K1T and the transposed gather call by call) against the
    literal rule on a contiguous Xᵀ; the reference's own mae knife-edge run (F16) reproduced through the pipeline."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    g = ROOT / "tests" / "golden"
    data, meta = np.load(g / "f16_mixed_transpose.npz"), json.loads((g / "golden_meta_f16.json").read_text())
    ref = next(r for r in meta["runs"] if r["run"] == "s100x150__thr_mae_knife_eq")
    x = data["s100x150__x"]
    xs = np.stack([x, x, scaled(0, 7950, (100, 150)), gen("heavy_f32", 7951, (100, 150))])   # the fixture twice: its knife-edge tile twice in a chunk
    xts = [np.ascontiguousarray(v.T) for v in xs]
    scores, _ = oracle_maps(xts[0], metric, [])
    thrs = knife_thresholds(scores, formats=["bfp8", "bfp4"], per_format=1) + ([ref["params"]["threshold"]] if metric == "mae" else [])
    xd = dev(xs, False)
    for thr in thrs:
        with ThresholdPipeline(ALL, metric, thr, chunk=chunk, layout="transpose") as pipe:
            if cap is not None:
                pipe.knife_cap = cap
            trips = spy_on_extra_trip(pipe)
            res = pipe.run(xd)
            assert pipe.knife_tiles > 0, (metric, thr, chunk, cap)
            if cap == 1:                              # the fixture's two copies share a chunk at either chunking: the extra trip ran
                assert pipe.knife_tiles > 1 and trips, (metric, thr, chunk, pipe.knife_tiles)
            else:
                assert not trips, (metric, thr, chunk, trips)
        for i, r in enumerate(res):
            a, counts, _sc = orc.threshold(xts[i], ALL, metric, thr)
            assert np.array_equal(r.assignment, a) and r.counts == counts, (metric, thr, chunk, cap, i)
            check_columns(r, xts[i], a, metric, True, (metric, thr, chunk, cap, i))
        if metric == "mae" and thr == ref["params"]["threshold"]:
            assert np.array_equal(res[0].assignment, data["s100x150__thr_mae_knife_eq__map"])
            assert [res[0].counts[f] for f in ALL] == ref["counts"]


@pytest.mark.parametrize("name", ["t_mae_130x200", "t_atol_130x200", "t_mae_split_heavy", "t_atol_split_heavy"])
def test_reference_fixtures_through_pipeline_and_plugin(golden_dir, name):
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    m = json.loads((golden_dir / "golden_meta.json").read_text())["f5"][name]
    d = np.load(golden_dir / "f5_threshold.npz")
    x, want = d[f"{name}_x"], d[f"{name}_assign"]
    assert m["metric"] in ("mae", "atol") and m["formats"] == ALL
    for chunk, count in ((4, 1), (4, 3), (2, 3)):        # alone; three copies in one chunk; in two chunks
        with ThresholdPipeline(ALL, m["metric"], m["threshold"], chunk=chunk) as pipe:
            res = pipe.run(dev(np.stack([x] * count), False))
        for r in res:
            assert np.array_equal(r.assignment, want) and [r.counts[f] for f in ALL] == d[f"{name}_counts"].tolist(), (name, chunk, count)
            check_columns(r, x, want, m["metric"], True, (name, chunk, count))
    for xin in (x, torch.from_numpy(x).cuda()):
        res = run_package_algo("mixed-tile-threshold", {"metric": m["metric"], "threshold": m["threshold"]}, xin, "hip")
        assert np.array_equal(res.meta["assignment"], want) and [res.tile_counts[f] for f in ALL] == d[f"{name}_counts"].tolist(), name


@pytest.mark.parametrize("metric", ["mae", "atol"])
def test_hip_plugin_on_every_input(metric):
    """The `hip` plugin (K1, K4 on the device, the literal re-scoring through K2) on every input and threshold of the table."""
    knives = 0
    for label, x, bf16 in tm.cases():
        knife, far = tm.thresholds(x, metric)
        _, wants = oracle_maps(x, metric, knife + [far])
        xin = dev(x, True) if bf16 else x
        for thr, want in zip(knife + [far], wants):
            with np.errstate(all="ignore"):
                res = run_package_algo("mixed-tile-threshold", {"metric": metric, "threshold": thr}, xin, "hip")
            assert np.array_equal(np.asarray(res.meta["assignment"]).reshape(want.shape), want), (label, metric, thr)
            assert (res.meta["knife_edge_tiles"] > 0) == (thr != far), (label, metric, thr)
            knives += res.meta["knife_edge_tiles"]
    assert knives > 0


@pytest.mark.parametrize("metric,lowest", [("mae", 0.01), ("atol", 0.04)])
def test_sweep_script_hip(tmp_path, metric, lowest):
    """scripts/sweep_mixed_tile_threshold.py --backend hip --metric mae | atol on the tiny preset's layer 0 (bf16 and float32 ragged
    matrices, an offset vector): step, threshold, size and tile counts of the reference's sweep on the oracle's literal scores."""
    from tests.test_configs_gpu import oracle_sweep

    out = tmp_path / "sweep"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "sweep_mixed_tile_threshold.py"), "synthetic:tiny", r"model\.layers\.0",
                        "--steps", "20", "--lowest-metric-val", str(lowest), "--backend", "hip", "--metric", metric, "--out-dir", str(out), "--no-plots"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    idx = model_source.build_model_index("synthetic:tiny")
    got = {p.parent.name: list(csv.reader(p.open())) for p in out.rglob("sweep_results.csv")}
    names = [n for n in idx.tensor_names if n.startswith("model.layers.0")]
    assert "model.layers.0.norm.weight" in names and len(got) == len(names)
    for name in names:
        x = np.asarray(idx.load(name).float().numpy(), dtype=np.float32)
        want = np.asarray(oracle_sweep(x, metric, lowest, 20))
        g = np.asarray([[float(v) for v in row] for row in got[name.replace("/", "_").replace(".", "_")][1:]])
        assert np.array_equal(g[:, :3], want[:, :3]), (metric, name)
        assert np.array_equal(g[:, 6:], want[:, 6:]), (metric, name)
        assert len(set(map(tuple, want[:, 6:]))) > 1, (metric, name)       # the sweep moves tiles between formats


@pytest.mark.parametrize("metric", ["mae", "atol"])
def test_wq_hip_with_a_metric_config(tmp_path, monkeypatch, capsys, metric):
    """wq --backend hip with {"metric": "mae" | "atol"} at a threshold ON a tile's float32 score: the tensors go through ThresholdPipeline
    (streamed.py hands it the config's metric); maps and printed tile counts are the literal rule's for every tensor."""
    from tests.test_configs_gpu import table_rows

    monkeypatch.chdir(tmp_path)
    idx = model_source.build_model_index("synthetic:tiny")
    names = model_source.resolve_selected_tensors(idx, None)
    xs = {n: np.asarray(idx.load(n).float().numpy(), dtype=np.float32) for n in names}
    s8 = orc.threshold_scores(xs["model.layers.0.attn.q.weight"], ALL, metric)["bfp8"]
    thr = float(np.sort(s8)[s8.size // 2])
    cfg = write_cfg(tmp_path, algo="mixed-tile-threshold", seed=None, params={"metric": metric, "threshold": thr})
    assert json.loads(Path(cfg).read_text())["params"]["threshold"] == thr
    assert cli.run(["synthetic:tiny", "--compression-config", cfg, "--backend", "hip", "--results-dir", str(tmp_path / "r"), "--no-plots"]) == 0
    assert re.search(r"streamed [1-9]\d* tensors in", capsys.readouterr().out)
    rdir = run_dir(tmp_path / "r")
    rows = table_rows((rdir / "table.txt").read_text())
    assert sorted(rows) == sorted(names)
    formats_seen = set()
    for n in names:
        with np.errstate(all="ignore"):
            want, counts, _sc = orc.threshold(xs[n], ALL, metric, thr)
        got = np.load(rdir / "mixed_tile_threshold" / cli._slug(n) / "assignment.npy")
        assert got.dtype == np.int8 and np.array_equal(got, want), n
        r = rows[n][("mixed-tile-threshold", "MIXED")]
        assert [int(v) for v in r[4:8]] == [counts[f] for f in ALL] and r[8] == round(orc.mixed_tile_total_bytes(counts)), n
        formats_seen |= {f for f in ALL if counts[f]}
    assert len(formats_seen) >= 2
