"""The threshold rule's knife-edge band on the GPU, on the inputs of tests/test_threshold_band.py (offset tensors, the float32
overflow / subnormal windows, degenerate, ragged and vector tiles): K4 on the device equals K4 on the host bit for bit (maps,
knife-edge sets and their format masks), and every device route — ThresholdPipeline.run and run_batches, the `hip` plugin,
the sweep script — gives the literal float32 rule's maps (orc.threshold)."""
import csv
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from tests.test_golden_r2 import run_package_algo
from tests.test_threshold_band import FIXED, degenerate_tensor, knife_thresholds, offset, oracle_maps, scaled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ALL = ["bf16", "bfp8", "bfp4", "bfp2"]


def inputs():
    """(label, float32 host values, bf16 storage?)"""
    out = [("offset100", offset(100.0, 0.5, (256, 256), 2), False), ("offset1000_bf16", offset(50.0, 0.05, (192, 256), 3, bf16=True), True),
           ("offset1", offset(0.05, 0.05, (128, 256), 4), False), ("degenerate", degenerate_tensor(), False),
           ("ragged_offset", offset(1.0, 0.01, (1000, 70), 5), False), ("ragged_33x17", scaled(0, 6, (33, 17)), False)]
    for k in (-80, -75, -70, -68, -66, -62, -50, 0, 50, 60, 63, 64, 66, 70, 75):
        out.append((f"2^{k}", scaled(k, seed=k + 1000, shape=(96, 128)), False))
    for k in (-70, 62, 66):
        out.append((f"heavy 2^{k}", scaled(k, seed=k + 3000, heavy=True), False))
    return out


def dev(x: np.ndarray, bf16: bool):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16).cuda() if bf16 else t.cuda()


@pytest.mark.parametrize("metric", ["pcc", "mae", "atol"])
def test_device_rule_equals_host_rule_bit_for_bit(metric):
    """threshold_assign_device against threshold_assign on the same device-written records: maps, knife ids, near masks —
    full records and (bf16 storage) the identity-bf16 records the pipelines decide on.  mae and atol (band·max(1, |threshold|), no
    moment widening): the inputs and thresholds of tests/test_threshold_metrics_host.py."""
    from tests import test_threshold_metrics_host as tm

    total_knife = 0
    for label, x, bf16 in (inputs() if metric == "pcc" else tm.cases()):
        x2d, _ = hb.to_device_2d(dev(x, bf16))
        layouts = [(0xF, 0xF)] + ([(0xE, 0xE | hb.MASK_BF16_IDENTITY)] if bf16 else [])
        if metric == "pcc":
            scores, _ = oracle_maps(x, "pcc", [])
            thresholds = list(FIXED) + knife_thresholds(scores, per_format=1)
        else:
            knife, far = tm.thresholds(x, metric)
            thresholds = knife + [far]
        for k1, dec in layouts:
            sdev = hb.tile_stats(x2d, k1)
            shost = sdev.cpu().numpy()
            for thr in thresholds:
                a_d, k_d, n_d = hb.threshold_assign_device(sdev, dec, ALL, metric, thr, 2e-6, with_near=True)
                a_h, k_h, n_h = hb.threshold_assign(shost, dec, ALL, metric, thr, 2e-6, with_near=True)
                assert np.array_equal(a_d, a_h) and np.array_equal(k_d, k_h) and np.array_equal(n_d, n_h), (label, hex(dec), thr)
                total_knife += k_d.size
    assert total_knife > 0


def test_threshold_pipeline_run_matches_literal_rule():
    """ThresholdPipeline.run on batches of offset and break-window matrices, knife_cap 1 included (more knife-edge tiles than the
    list holds: every tile of a break-window matrix is one)."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    batches = [("offset", np.stack([offset(100.0, 0.5, (96, 160), 10 + i) for i in range(3)]), False),
               ("offset_bf16", np.stack([offset(1.0, 0.01, (128, 256), 20 + i, bf16=True) for i in range(3)]), True),
               ("windows", np.stack([scaled(k, seed=300 + k, shape=(96, 160)) for k in (66, -68, 0, 64)]), False)]
    for label, xs, bf16 in batches:
        scores, _ = oracle_maps(xs[0], "pcc", [])
        for thr in (0.99, 0.999) + tuple(knife_thresholds(scores, formats=["bfp8", "bfp4"], per_format=1, ulps=False)):
            for cap in (None, 1):
                pipe = ThresholdPipeline(ALL, "pcc", thr, chunk=2)
                if cap is not None:
                    pipe.knife_cap = cap
                with np.errstate(all="ignore"):
                    res = pipe.run(dev(xs, bf16))
                    for i, r in enumerate(res):
                        a, counts, _sc = orc.threshold(xs[i], ALL, "pcc", thr)
                        assert np.array_equal(r.assignment, a) and r.counts == counts, (label, thr, cap, i)
                pipe.close()


def test_threshold_run_batches_ragged_mix_with_offset_vectors():
    """run_batches over a ragged mix: offset vectors (the layer-norm weights of the presets, as (n/32, 32) matrices with their element
    counts), offset and break-window matrices, two storage types; every map the literal rule's."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    vecs = [offset(1.0, 0.01, (n,), 40 + n, bf16=True) for n in (512, 1000, 1536)]
    mats = [(offset(100.0, 0.5, (70, 100), 50), False), (scaled(66, 51, (64, 96)), False), (scaled(-68, 52, (33, 17)), False),
            (offset(10.0, 0.05, (96, 160), 53, bf16=True), True), (scaled(0, 54, (128, 128)), True)]
    batches, hosts = [], []
    for v in vecs:
        vm = np.zeros((-(-v.size // 32) * 32,), dtype=np.float32)     # ceil(n/32) rows of 32, the last one zero-filled
        vm[: v.size] = v
        batches.append((dev(vm, True).view(1, -1, 32), v.size))
        hosts.append(v)
    for m, bf16 in mats:
        batches.append((dev(m, bf16)[None], None))
        hosts.append(m)
    scores, _ = oracle_maps(hosts[3], "pcc", [])
    for thr in (0.999, float(np.sort(scores["bfp8"])[len(scores["bfp8"]) // 2])):
        with ThresholdPipeline(ALL, "pcc", thr, chunk=2) as pipe:
            with np.errstate(all="ignore"):
                got = pipe.run_batches(batches)
        for i, h in enumerate(hosts):
            with np.errstate(all="ignore"):
                a, counts, _sc = orc.threshold(h, ALL, "pcc", thr)
            assert np.array_equal(got[i][0].assignment.reshape(-1), a.reshape(-1)) and got[i][0].counts == counts, (thr, i)


def test_hip_plugin_matches_literal_rule():
    for label, x, bf16 in inputs():
        scores, wants = oracle_maps(x, "pcc", [])
        thrs = list(FIXED) + knife_thresholds(scores, per_format=1)
        _, wants = oracle_maps(x, "pcc", thrs)
        xin = torch.from_numpy(x).to(torch.bfloat16).cuda() if bf16 else x
        for thr, want in zip(thrs, wants):
            with np.errstate(all="ignore"):
                res = run_package_algo("mixed-tile-threshold", {"metric": "pcc", "threshold": thr}, xin, "hip")
            assert np.array_equal(np.asarray(res.meta["assignment"]).reshape(want.shape), want), (label, thr)


def test_sweep_script_hip_on_offset_tensors(tmp_path):
    """scripts/sweep_mixed_tile_threshold.py --backend hip on the tiny preset (an offset `ones` vector among ragged matrices and
    a vector): start threshold, per-step thresholds, sizes and tile counts of the reference's sweep on the oracle's scores."""
    from quantization_analysis_amd import model_source
    from tests.test_configs_gpu import oracle_sweep

    out = tmp_path / "sweep"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "sweep_mixed_tile_threshold.py"), "synthetic:tiny", r"model\.layers\.0",
                        "--steps", "30", "--lowest-metric-val", "0.9", "--backend", "hip", "--out-dir", str(out), "--no-plots"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    idx = model_source.build_model_index("synthetic:tiny")
    got = {p.parent.name: list(csv.reader(p.open())) for p in out.rglob("sweep_results.csv")}
    names = [n for n in idx.tensor_names if n.startswith("model.layers.0")]
    assert "model.layers.0.norm.weight" in names and len(got) == len(names)
    for name in names:
        x = np.asarray(idx.load(name).float().numpy(), dtype=np.float32)
        want = np.asarray(oracle_sweep(x, "pcc", 0.9, 30))
        g = np.asarray([[float(v) for v in row] for row in got[name.replace("/", "_").replace(".", "_")][1:]])
        assert np.array_equal(g[:, :3], want[:, :3]), name
        assert np.array_equal(g[:, 6:], want[:, 6:]), name
