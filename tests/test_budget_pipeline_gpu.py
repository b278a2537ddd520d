"""mixed-tile-budget on the MI355X above the C ABI: BudgetPipeline, the hip plugin, wq's streamed route and pack_model.py in both scopes.
The device allocation is compared with budget_maps.allocate on the pipeline's own device table (equal tables give equal maps); hip and
emulation are compared where their tables are equal by construction, on the exact-sum inputs of tests/test_calibration_exact_host.py."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import cli, packed
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms import create_algorithm
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import columns_from_stats, compute_tile_stats
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS, mixed_tile_total_bytes
from quantization_analysis_amd.model_source import build_model_index
from quantization_analysis_amd.pipeline import BudgetPipeline
from tests.test_calibration_exact_host import tables_weight
from tests.test_packed_batch_host import pack_model_script

pytestmark = pytest.mark.gpu
ALL = list(MIXED_TILE_FORMATS)
EXAMPLE = "compression_config.mixed_tile_budget.example.json"


def _root():
    from pathlib import Path

    return Path(__file__).resolve().parent.parent


def _batch(dtype, count=5, rows=128, cols=192, seed=0):
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((count, rows, cols), generator=g, device="cuda") * 0.05
    x[:, ::3, ::5] *= 20.0                                           # tiles of very different sensitivity
    x = x * torch.linspace(0.2, 3.0, count, device="cuda")[:, None, None]
    return x.to(dtype)


def _cache(tmp_path, backend):
    return CacheContext(tmp_path / "cache", "t", backend, True, "t")


@pytest.mark.parametrize("bits,formats", [(4.5, ALL), (2.5, ALL), (9.0, ALL), (6.0, ["bf16", "bfp8", "bfp4"]), (16.0, ALL)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pipeline_maps_equal_allocate_on_its_own_table(dtype, bits, formats):
    x = _batch(dtype)
    with BudgetPipeline(formats, "pcc", bits, pure_formats=formats) as pipe:
        res = pipe.run(x)
        table = pipe.table_dev.cpu().numpy().copy()
        maps_dev = pipe.maps_dev.cpu().numpy().copy()
    assert table.shape == (5, 24, 4) and len(res) == 5
    q = Quantizer("hip")
    for j, r in enumerate(res):
        want_a, want_counts, want_bytes = bm.allocate(table[j], formats, bits, (4, 6))
        assert np.array_equal(r.assignment, want_a) and np.array_equal(maps_dev[j].reshape(4, 6), want_a), (j, bits)
        assert r.counts == want_counts and r.tile_bytes == want_bytes == mixed_tile_total_bytes(want_counts)
        assert r.tile_bytes <= bits / 8.0 * 1024.0 * 24
        ts = compute_tile_stats(x[j], formats, q)
        c = columns_from_stats(ts, want_a)
        assert (r.pcc, r.mae, r.atol) == (c["pcc"], c["mae"], c["atol"]) and r.metric_value == c["pcc"]
        for f in formats:                                            # wq's `none` rows from the same records
            pc = columns_from_stats(ts, np.full((4, 6), ALL.index(f), dtype=np.int8))
            assert r.pure[f] == (pc["pcc"], pc["mae"], pc["atol"]), (j, f)
    if bits == 16.0:
        assert all(r.counts["bf16"] > 0 for r in res)


def test_run_batches_equals_run_and_a_refused_tensor_raises_the_reason():
    a, b = _batch(torch.bfloat16, count=3), _batch(torch.float32, count=2, rows=70, cols=100, seed=1)
    with BudgetPipeline(ALL, "mae", 5.0) as pipe:
        one = [pipe.run(a), pipe.run(b)]
        both = pipe.run_batches([a, (b, None)])
    for r1, r2 in zip(one[0] + one[1], both[0] + both[1]):
        assert np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts and r1.metric_value == r2.metric_value == r1.mae
    with BudgetPipeline(ALL, "pcc", 1.5) as pipe:
        with pytest.raises(ValueError, match="tensor 0 of the batch: budget .* is below the all-bfp2 size"):
            pipe.run(a)
    bad = a.float()
    bad[1, 5, 7] = float("inf")
    with BudgetPipeline(ALL, "pcc", 5.0) as pipe:
        with pytest.raises(ValueError, match="tensor 1 of the batch: the tile error table holds a non-finite value"):
            pipe.run(bad)


def _exact_tensors():
    """Tensors whose tables are exact in any summation order: hip and emulation then hold the same table, hence the same map."""
    out = {}
    for i, (n, k, wdt) in enumerate([(96, 160, "bf16"), (70, 100, "f32"), (96, 160, "f32"), (64, 96, "bf16")]):
        w = np.ascontiguousarray(tables_weight(n, k, i)[:, 2: 2 + k])
        t = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32)
        assert np.array_equal(t.float().numpy().view(np.uint32), w.view(np.uint32))
        out[f"exact.{i}.weight"] = t
    return out


@pytest.mark.parametrize("bits", [3.0, 4.5, 7.0])
def test_exact_sum_inputs_give_the_emulation_backends_maps(tmp_path, bits):
    torch.cuda.set_device(0)
    algo = create_algorithm("mixed-tile-budget", {"bits": bits})
    for name, t in _exact_tensors().items():
        emu = algo.run(t.float().numpy(), ALL, Quantizer("emulation"), _cache(tmp_path, "emulation"))[0]
        with BudgetPipeline(ALL, "pcc", bits) as pipe:
            r = pipe.run(t.cuda()[None])[0]
        assert np.array_equal(r.assignment, emu.meta["assignment"]) and r.counts == emu.tile_counts and r.tile_bytes == emu.tile_bytes, name
        plug = algo.run(t.cuda(), ALL, Quantizer("hip"), _cache(tmp_path, "hip"))[0]
        assert np.array_equal(plug.meta["assignment"], emu.meta["assignment"]) and plug.meta["predicted_sse"] == emu.meta["predicted_sse"], name


@pytest.mark.parametrize("shape", [(1000,), (3, 40, 50)], ids=["vector", "rank3"])
def test_the_hip_plugin_per_tensor(tmp_path, shape):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(len(shape))
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    w.reshape(-1)[::37] *= 25.0
    x = torch.from_numpy(w).cuda()
    algo = create_algorithm("mixed-tile-budget", {"bits": 5.0, "metric": "mae"})
    q = Quantizer("hip")
    r = algo.run(x, ALL, q, _cache(tmp_path, "hip"))[0]
    assert r.fmt == "MIXED" and r.compression == "mixed-tile-budget" and tuple(r.y.shape) == shape
    ts = compute_tile_stats(x, ALL, q)
    table = hb.tile_sq_error_batched(ts.x2d)[0].cpu().numpy()
    want_a, want_counts, want_bytes = bm.allocate(table, ALL, 5.0, (ts.tiles_h, ts.tiles_w))
    assert np.array_equal(r.meta["assignment"], want_a) and r.tile_counts == want_counts and r.tile_bytes == want_bytes
    assert r.meta["columns"] == columns_from_stats(ts, want_a) and r.meta["predicted_sse"] == bm.predicted_sse(table, want_a)
    assert r.meta["bits"] == 5.0 and r.meta["budget_bytes"] == 5.0 / 8.0 * 1024.0 * ts.tiles and r.meta["tile_formats"] == ALL
    y = r.y.cpu().numpy().astype(np.float64)
    assert np.isclose(((y - w.astype(np.float64)) ** 2).sum(), r.meta["predicted_sse"], rtol=1e-9)
    with pytest.raises(ValueError, match="below the all-bfp2 size"):
        create_algorithm("mixed-tile-budget", {"bits": 1.0}).run(x, ALL, q, _cache(tmp_path, "hip"))


def _write_cfg(tmp_path, **params):
    cfg = json.loads((_root() / "compression_configs" / EXAMPLE).read_text())
    cfg["params"].update(params)
    path = tmp_path / f"cfg_{'_'.join(f'{k}{v}' for k, v in params.items()) or 'example'}.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def test_wq_streams_the_example_config(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    cfg = str(_root() / "compression_configs" / EXAMPLE)
    assert cli.run(["synthetic:tiny", "--compression-config", cfg, "--backend", "hip", "--results-dir", str(tmp_path / "res")]) == 0
    tables = list((tmp_path / "res").rglob("table.txt"))
    assert len(tables) == 1 and "mixed-tile-budget" in str(tables[0])
    text = tables[0].read_text()
    assert text.count("MIXED") >= 5 and "mixed-tile-budget" in text
    art = tables[0].parent / "mixed_tile_budget"
    assert len(list(art.rglob("*.npy"))) == 5 and len(list(art.rglob("*.json"))) >= 5 and len(list(art.rglob("*.png"))) >= 5
    idx = build_model_index("synthetic:tiny")
    q = Quantizer("hip")
    for npy in art.rglob("*.npy"):                                   # every written map is allocate's on the tensor's device table
        amap = np.load(npy)
        name = next(n for n in idx.specs if cli._slug(n) == npy.parent.name)
        ts = compute_tile_stats(idx.load(name, device=torch.device("cuda", 0)), ALL, q)
        table = hb.tile_sq_error_batched(ts.x2d)[0].cpu().numpy()
        assert np.array_equal(amap, bm.allocate(table, ALL, 4.5, (ts.tiles_h, ts.tiles_w))[0]), name
    capsys.readouterr()
    assert cli.run(["synthetic:tiny", "--compression-config", _write_cfg(tmp_path, scope="model"), "--backend", "hip",
                    "--results-dir", str(tmp_path / "res2"), "--no-plots"]) == 1
    assert "pack_model.py" in capsys.readouterr().err


def test_a_transpose_layout_config_is_refused(tmp_path, capsys):
    with pytest.raises(ValueError, match="row layout only"):
        create_algorithm("mixed-tile-budget", {"bits": 4.5, "layout": "transpose"})
    script = pack_model_script()
    assert script.main(["synthetic:tiny", "--compression-config", _write_cfg(tmp_path, layout="transpose"), "--out-dir", str(tmp_path / "o"),
                        "--backend", "hip"]) == 1
    assert "row layout only" in capsys.readouterr().out


def _device_tables(index, names):
    """Every tensor's device table and tile grid, tensor by tensor."""
    tables, grids = [], []
    for n in names:
        x2d, _info = hb.to_device_2d(index.load(n, device=torch.device("cuda", 0)))
        tables.append(hb.tile_sq_error_batched(x2d)[0].cpu().numpy())
        grids.append(hb.tiles_hw(*x2d.shape))
    return tables, grids


@pytest.mark.parametrize("scope", ["tensor", "model"])
def test_pack_model_on_hip(tmp_path, capsys, scope):
    torch.cuda.set_device(0)
    script = pack_model_script()
    out = tmp_path / scope
    assert script.main(["synthetic:tiny", "--compression-config", _write_cfg(tmp_path, scope=scope), "--out-dir", str(out), "--backend", "hip",
                        "--verify"]) == 0
    text = capsys.readouterr().out
    assert "verify: ok (5 tensors" in text and "MISMATCH" not in text and f"scope {scope}" in text and "bits per weight" in text
    index = json.loads((out / "index.json").read_text())
    run = index["run"]
    names = list(index["tensors"])
    got = packed.load_dir(out)
    model_index = build_model_index("synthetic:tiny")
    tables, grids = _device_tables(model_index, names)
    tiles = sum(th * tw for th, tw in grids)
    achieved = mixed_tile_total_bytes({f: sum(e["counts"][f] for e in index["tensors"].values()) for f in ALL})
    assert run["bits"] == 4.5 and run["scope"] == scope and run["size_model_bytes"] == achieved
    assert run["budget_bytes"] == 4.5 / 8.0 * 1024.0 * tiles and achieved <= run["budget_bytes"]
    assert abs(run["achieved_bits"] - achieved * 8.0 / (1024.0 * tiles)) < 1e-12 and run["achieved_bits"] <= 4.5
    assert all(e["verified"] is True for e in index["tensors"].values())
    if scope == "model":
        maps, counts, size = bm.model_maps(tables, grids, ALL, 4.5)
        assert size == achieved
        for n, want in zip(names, maps):
            assert np.array_equal(got[n].map, want), n
        assert sorted(e["route"] for e in index["tensors"].values()).count("model-scope batched") == 4
    else:
        for n, t, g in zip(names, tables, grids):
            assert np.array_equal(got[n].map, bm.allocate(t, ALL, 4.5, g)[0]), n
        assert sorted(e["route"] for e in index["tensors"].values()).count("batched") == 4


@pytest.mark.parametrize("scope", ["tensor", "model"])
def test_pack_model_on_exact_sum_inputs_equals_the_emulation_run(tmp_path, capsys, scope):
    from safetensors.torch import save_file

    torch.cuda.set_device(0)
    model = tmp_path / "model"
    model.mkdir()
    save_file(_exact_tensors(), str(model / "model.safetensors"))
    script = pack_model_script()
    cfg = _write_cfg(tmp_path, scope=scope, bits=4.0)
    for backend in ("hip", "emulation"):
        assert script.main([str(model), "--compression-config", cfg, "--out-dir", str(tmp_path / backend), "--backend", backend, "--verify"]) == 0
    assert "MISMATCH" not in capsys.readouterr().out
    hip, emu = packed.load_dir(tmp_path / "hip"), packed.load_dir(tmp_path / "emulation")
    assert list(hip) == list(emu) and len(hip) == 4
    for n in hip:
        assert np.array_equal(hip[n].map, emu[n].map) and np.array_equal(hip[n].data, emu[n].data), n
    runs = [json.loads((tmp_path / b / "index.json").read_text())["run"] for b in ("hip", "emulation")]
    assert runs[0]["size_model_bytes"] == runs[1]["size_model_bytes"] <= runs[0]["budget_bytes"] == runs[1]["budget_bytes"]
