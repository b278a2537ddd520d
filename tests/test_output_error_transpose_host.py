"""Layer-output error in the transposed BFP layout on the host: the emulation's +transpose rows against a direct float64 X·Ŵᵀ, the
rows and their order through evaluate_op and the CLI, the transposed tables against a brute-force einsum, the saved transposed maps
through reconstruct_mixed_tile_assignment.py --layout transpose, GPTQ's skip entries and the new C entry points' argument checks."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.config import CompressionConfig
from quantization_analysis_amd.layer_io import Chunk, select_ops
from quantization_analysis_amd.model_source import build_model_index
from quantization_analysis_amd.output_error import (LAYOUTS, SLOTS, check_layout, emulation_sums, evaluate_op, quantize_transposed,
                                                    quantize_x, search_map)
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen
from tests.test_output_error_host import make_fixture

ROOT = Path(__file__).resolve().parent.parent
FMTS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
TF = ["bfp8", "bfp4", "bfp2"]
T0 = len(SLOTS)


def _direct(x64, what, bias, r):
    """The seven sums of one candidate computed directly in float64."""
    q = x64 @ what.T + (0.0 if bias is None else bias)
    d = np.abs(r - q)
    return np.array([r.sum(), (r * r).sum(), q.sum(), (q * q).sum(), (r * q).sum(), d.sum(), d.max()])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 50])
@pytest.mark.parametrize("k,with_bias,x_format", [(40, False, "bf16"), (33, True, "bf16"), (70, True, "bfp8")])
def test_emulation_transposed_rows_match_direct(n, k, with_bias, x_format):
    w = gen("heavy_f32", n * 100 + k, (n, k))
    x = torch.from_numpy(gen("normal_bf16", n + k, (23, k)) * 10).to(torch.bfloat16)
    bias = gen("normal_f32", 3, (n,)).astype(np.float64) if with_bias else None
    sums, m, _seen, _cast = emulation_sums([Chunk(x=x[:9]), Chunk(x=x[9:])], torch.from_numpy(w), [], None if bias is None else torch.from_numpy(bias),
                                           x_format=x_format, t_formats=TF)
    assert m == 23 and sums.shape == (2 * len(SLOTS), 7)
    x64 = x.double().numpy()
    r = x64 @ w.astype(np.float64).T + (0.0 if bias is None else bias)
    xq = x64 if x_format == "bf16" else quantize_x(x, x_format).numpy()
    for f in TF:
        what = quantize_weight_values(np.ascontiguousarray(w.T), f).T.astype(np.float64)
        # the group is 16 consecutive rows of one column, a ragged last group completed with +0
        wp = np.zeros((-(-n // 16) * 16, k), np.float32)
        wp[:n] = w
        assert np.array_equal(what, quantize_weight_values(np.ascontiguousarray(wp.T), f).T[:n].astype(np.float64))
        np.testing.assert_allclose(sums[T0 + SLOTS.index(f)], _direct(xq, what, bias, r), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(sums[T0 + SLOTS.index("fp0")], sums[SLOTS.index("fp0")], rtol=0, atol=0)


def test_check_layout_opt_in():
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"layout": "transpose"}, quantization_formats=None, seed=None, random_seed=False)
    with pytest.raises(ValueError, match="row layout"):
        check_layout(cfg)
    check_layout(cfg, LAYOUTS)
    check_layout(CompressionConfig(algorithm="transpose", params={}, quantization_formats=None, seed=None, random_seed=False), LAYOUTS)


def _ops(tmp_path):
    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp", "test")
    cal, _ = select_ops(index, io, "model.layers.0.mlp", "calibration")
    return model, io, index, ops, {o.op: o for o in cal}


def test_evaluate_op_transpose_config_rows(tmp_path):
    """A config with the transpose algorithm implies the transposed rows; each equals the transpose algorithm's y through the LOE."""
    _model, _io, index, ops, _cal = _ops(tmp_path)
    cfg = CompressionConfig(algorithm="transpose", params={}, quantization_formats=FMTS, seed=None, random_seed=False)
    for op in ops:
        res = evaluate_op(index, op, FMTS, cfg)
        assert [r.candidate for r in res.rows] == FMTS + [f + "+transpose" for f in TF] + ["recorded"]
        plain = evaluate_op(index, op, FMTS)
        assert [(r.candidate, r.bytes, r.pcc, r.mae, r.atol) for r in plain.rows if not r.candidate.endswith("+transpose")] == \
               [(r.candidate, r.bytes, r.pcc, r.mae, r.atol) for r in res.rows if not r.candidate.endswith("+transpose")]
        w = index.load(op.weight)
        n, k = res.shape
        from quantization_analysis_amd.compression_algorithms import create_algorithm
        from quantization_analysis_amd.compression_algorithms.cache import CacheContext
        from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer

        ys = {r.fmt.lower(): r.y for r in create_algorithm("transpose", {}).run(xf=w.float().numpy(), formats=TF, quantizer=Quantizer("emulation"),
                                                                          cache=CacheContext(root=tmp_path / "c", tensor_name=op.weight,
                                                                                             backend="emulation", recompute=True, run_tag="t"))}
        for f in TF:
            row = next(r for r in res.rows if r.candidate == f + "+transpose")
            assert row.extra == {"layout": "transpose"} and row.bytes == next(r for r in res.rows if r.candidate == f).bytes
            y = np.asarray(ys[f].float().numpy() if hasattr(ys[f], "numpy") else ys[f], np.float32)
            assert np.array_equal(y.view(np.uint32), quantize_transposed(w.float().numpy(), f).view(np.uint32))
            from quantization_analysis_amd.layer_io import chunks
            s, *_ = emulation_sums(chunks(op, k, n, 16384), w, [], index.load(op.bias) if op.bias else None, y)
            assert row.sums == tuple(s[SLOTS.index("map")])


def test_evaluate_op_transposed_greedy_map(tmp_path):
    """A "layout": "transpose" greedy config: map:mixed-tile-greedy+transpose over Wᵀ's grid, equal to the LOE of the search's y."""
    _model, _io, index, ops, _cal = _ops(tmp_path)
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"metric": "pcc", "threshold": 0.999, "layout": "transpose"},
                            quantization_formats=FMTS, seed=123, random_seed=False)
    for op in ops:
        res = evaluate_op(index, op, FMTS, cfg)
        assert [r.candidate for r in res.rows] == FMTS + ["map:mixed-tile-greedy+transpose", "recorded"]
        n, k = res.shape
        w = index.load(op.weight)
        mc = search_map(w, cfg, "emulation", op.weight)
        assert mc.layout == "transpose" and mc.assignment.shape == bm.tiles_hw(k, n)
        from quantization_analysis_amd.layer_io import chunks
        s, *_ = emulation_sums(chunks(op, k, n, 16384), w, [], index.load(op.bias) if op.bias else None, mc.y)
        row = res.rows[len(FMTS)]
        assert row.sums == tuple(s[SLOTS.index("map")]) and row.bytes == mc.tile_bytes and row.extra == {"layout": "transpose"}
        assert np.array_equal(bm.reconstruct_emulation(w, mc.assignment, "transpose").view(np.uint32),
                              np.asarray(mc.y, np.float32).view(np.uint32))


@pytest.mark.parametrize("n,k", [(70, 100), (33, 7), (64, 96), (1, 40)])
def test_transposed_tables_match_brute_force(n, k):
    w = gen("heavy_f32", n + k, (n, k))
    w[:16, 3] = 0.0
    x = gen("normal_bf16", 2, (50, k)).astype(np.float64)
    tk, tn = bm.tiles_hw(k, n)
    xp = np.zeros((50, tk * 32))
    xp[:, :k] = x
    h = np.einsum("mbi,mbj->bij", xp.reshape(50, tk, 32), xp.reshape(50, tk, 32))
    e_out, e_w = bm.tile_error_tables_emulation(w, h, "transpose")
    for code, f in enumerate(TF + ["bf16"]):
        code = ["bf16", "bfp8", "bfp4", "bfp2"].index(f)
        delta = quantize_transposed(w, f).astype(np.float64) - w.astype(np.float64)
        for r in range(tk):
            for c in range(tn):
                d = np.zeros((32, 32))                                   # rows of W in the tile × columns of block r
                blk = delta[32 * c: 32 * c + 32, 32 * r: 32 * r + 32]
                d[: blk.shape[0], : blk.shape[1]] = blk
                t = r * tn + c
                want = sum(d[i] @ h[r] @ d[i] for i in range(32))
                assert abs(e_out[t, code] - want) <= 1e-12 * abs(want) + 1e-300
                assert abs(e_w[t, code] - (d * d).sum()) <= 1e-12 * (d * d).sum() + 1e-300


def _run(args):
    return subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), *args], capture_output=True, text=True,
                          cwd=ROOT, timeout=600)


def test_cli_transpose_budget_maps_and_row_order(tmp_path):
    model, io = make_fixture(tmp_path)
    base = [str(model), str(io), "model.layers.0", "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--split", "test",
            "--budget-bits", "3", "4.5"]
    r0 = _run(base + ["--out-dir", str(tmp_path / "plain")])
    r1 = _run(base + ["--out-dir", str(tmp_path / "t"), "--transpose", "--save-maps"])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    d0 = json.loads((tmp_path / "plain" / "layer_output_error.json").read_text())
    d1 = json.loads((tmp_path / "t" / "layer_output_error.json").read_text())
    assert "transpose" not in d0 and d1["transpose"] is True
    for o0, o1 in zip(d0["ops"], d1["ops"]):
        names = [x["candidate"] for x in o1["rows"]]
        assert names == ["bf16", "bfp8", "bfp4", "bfp2", "fp0", "bfp8+transpose", "bfp4+transpose", "bfp2+transpose", "recorded",
                         "budget:3:output", "budget:3:weight", "budget:3:output+transpose", "budget:3:weight+transpose",
                         "budget:4.5:output", "budget:4.5:weight", "budget:4.5:output+transpose", "budget:4.5:weight+transpose"]
        # --transpose only adds rows: every row-layout row as without it, in the same relative order
        assert [x for x in o1["rows"] if x.get("layout") != "transpose"] == o0["rows"]
        for x in o1["rows"]:
            if x["candidate"].endswith("+transpose"):
                assert x["layout"] == "transpose"
    op = "model.layers.0.mlp.down_proj"
    from safetensors.torch import load_file

    w = load_file(str(model / "m.safetensors"))[f"{op}.weight"]
    n, k = w.shape
    for basis in ("output", "weight"):
        npy = tmp_path / "t" / "maps" / op / f"budget_4.5_{basis}_transpose.npy"
        a = np.load(npy)
        assert a.dtype == np.int8 and a.shape == bm.tiles_hw(k, n)
        assert (tmp_path / "t" / "maps" / op / f"budget_4.5_{basis}.npy").exists()
        out = tmp_path / f"recon_{basis}.npy"
        rr = subprocess.run([sys.executable, str(ROOT / "scripts" / "reconstruct_mixed_tile_assignment.py"), str(model), f"{op}.weight",
                             str(npy), "--layout", "transpose", "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert rr.returncode == 0, rr.stderr
        assert np.array_equal(np.load(out).view(np.uint32), bm.reconstruct_emulation(w, a, "transpose").view(np.uint32))


def test_cli_output_unchanged_without_transpose(tmp_path):
    """Without --transpose and without a transposed config the new code adds nothing: the transposed greedy config is the only
    route to a map+transpose row, and its row-layout rows match the row config's pure-format rows."""
    model, io = make_fixture(tmp_path)
    base = [str(model), str(io), "model.layers.0.mlp", "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "fp0", "--split", "test"]
    r = _run(base + ["--out-dir", str(tmp_path / "a"), "--compression-config",
                     str(ROOT / "compression_configs" / "compression_config.mixed_tile_greedy_transpose.example.json")])
    assert r.returncode == 0, r.stderr
    doc = json.loads((tmp_path / "a" / "layer_output_error.json").read_text())
    assert "transpose" not in doc
    for o in doc["ops"]:
        assert [x["candidate"] for x in o["rows"]] == ["bf16", "bfp8", "bfp4", "fp0", "map:mixed-tile-greedy+transpose", "recorded"]


def test_gptq_skips_transposed_candidates(tmp_path):
    _model, _io, index, ops, cal = _ops(tmp_path)
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"metric": "pcc", "threshold": 0.999, "layout": "transpose"},
                            quantization_formats=FMTS, seed=123, random_seed=False)
    for op in ops:
        res = evaluate_op(index, op, ["bf16", "bfp8", "bfp4"], cfg, budgets=(9,), calib=cal[op.op], gptq=True, transpose=True)
        names = [r.candidate for r in res.rows]
        assert [c for c in names if c.startswith("gptq:")] == ["gptq:bfp8", "gptq:bfp4", "gptq:budget:9:output"]
        skipped = dict(res.budget_skipped)
        for c in ("gptq:bfp8+transpose", "gptq:bfp4+transpose", "gptq:map:mixed-tile-greedy+transpose", "gptq:budget:9:output+transpose"):
            assert "row-layout only" in skipped[c], (c, skipped)


def test_c_entry_points_check_arguments():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    sz = L.mtq_output_error_scratch_doubles(4, 50)
    oe = L.mtq_output_error_transposed
    assert oe(None, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, None, 0) == -1
    assert b"null" in L.mtq_last_error()
    assert oe(p, 4, 40, 40, p, 0, 50, 40, None, 0x1F, None, None, 0, 0, p, p, sz, None, None, 0) == -4   # format bit 4
    assert oe(p, 4, 40, 40, p, 7, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, None, 0) == -1    # w dtype
    assert oe(p, 4, 40, 39, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, None, 0) == -1
    assert b"ldx < k" in L.mtq_last_error()
    assert oe(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, 1, None, None, 0) == -1
    assert b"scratch" in L.mtq_last_error()
    assert oe(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, p, 39) == -1
    assert b"ldxq < k" in L.mtq_last_error()
    assert oe(p, 0, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, None, 0) == -1
    te = L.mtq_tile_error_tables_transposed
    tk, tn = hb.tiles_hw(40, 50)
    assert te(None, 0, 50, 40, 40, p, tk * 1024, p, p, tk * tn * 4, None) == -1 and b"null" in L.mtq_last_error()
    assert te(p, 7, 50, 40, 40, p, tk * 1024, p, p, tk * tn * 4, None) == -1
    assert te(p, 0, 50, 40, 39, p, tk * 1024, p, p, tk * tn * 4, None) == -1 and b"ldw < k" in L.mtq_last_error()
    assert te(p, 0, 50, 40, 40, p, tk * 1024 + 1, p, p, tk * tn * 4, None) == -1 and b"h_doubles" in L.mtq_last_error()
    assert te(p, 0, 50, 40, 40, p, tk * 1024, p, p, tk * tn * 4 + 4, None) == -1 and b"table_doubles" in L.mtq_last_error()
    assert te(p, 0, 0, 40, 40, p, tk * 1024, p, p, tk * tn * 4, None) == -1
