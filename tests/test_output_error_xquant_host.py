"""Layer-output error with BFP-quantised activations (x_format) on the host: the float64 emulation against a direct computation,
the default's bits, chunk invariance of Q(X), the refusals of the Python and C entry points, and the CLI's --x-format."""
from __future__ import annotations

import csv
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.layer_io import Chunk, select_ops
from quantization_analysis_amd.model_source import build_model_index
from quantization_analysis_amd.output_error import SLOTS, X_FORMATS, emulation_sums, evaluate_op, hip_sums, quantize_x
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen
from tests.test_output_error_host import _direct, make_fixture

ROOT = Path(__file__).resolve().parent.parent
FMTS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]


def _direct_qx(x, qx, w, bias, wq):
    """float64 sums of Y = Q(X)·Ŵᵀ + b (Y = b for wq None) against R = X·Wᵀ + b."""
    x64 = np.asarray(x, dtype=np.float64)
    r = x64 @ np.asarray(w, dtype=np.float64).T
    q = np.asarray(qx, dtype=np.float64) @ np.asarray(wq, dtype=np.float64).T if wq is not None else np.zeros_like(r)
    if bias is not None:
        r = r + bias
        q = q + bias
    d = np.abs(r - q)
    return np.array([r.sum(), (r * r).sum(), q.sum(), (q * q).sum(), (r * q).sum(), d.sum(), d.max()])


def _x(m, k, seed):
    """bf16 activations whose 16-groups mix magnitudes, so every BFP format rounds and drops elements."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, k)) * np.exp2(rng.integers(-6, 7, (m, k)))
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16)


@pytest.mark.parametrize("x_format", X_FORMATS)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", ["heavy_bf16", "normal_f32"])
def test_emulation_matches_direct_float64(kind, with_bias, x_format):
    n, k, m = 50, 70, 37
    w = gen(kind, 3, (n, k))
    x = _x(m, k, 4)
    bias = gen("normal_f32", 5, (n,)) if with_bias else None
    amap = np.random.default_rng(6).integers(0, 4, size=(2, 3))
    my = np.zeros_like(w)
    for ti in range(2):
        for tj in range(3):
            sl = np.s_[ti * 32:(ti + 1) * 32, tj * 32:(tj + 1) * 32]
            my[sl] = quantize_weight_values(w[sl], ["bf16", "bfp8", "bfp4", "bfp2"][amap[ti, tj]])
    sums, mm, rec, cast = emulation_sums([Chunk(x=x[:20]), Chunk(x=x[20:])], w, FMTS, bias, my, x_format=x_format)
    assert mm == m and not rec and not cast
    xf = x.float().numpy()
    qx = quantize_weight_values(xf, x_format)
    if x_format != "bf16":
        assert not np.array_equal(qx, xf)
    for f in FMTS:
        want = _direct_qx(xf, qx, w, bias, None if f == "fp0" else quantize_weight_values(w, f))
        np.testing.assert_allclose(sums[SLOTS.index(f)], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    np.testing.assert_allclose(sums[SLOTS.index("map")], _direct_qx(xf, qx, w, bias, my), rtol=1e-12)
    # fp0 does not see Q(X): Y = b against the raw R, as without an activation format
    np.testing.assert_allclose(sums[SLOTS.index("fp0")], _direct(xf, w, bias, None), rtol=1e-12)


@pytest.mark.parametrize("kind", ["heavy_bf16", "normal_f32"])
def test_bf16_x_format_is_the_default_bit_for_bit(kind):
    w = gen(kind, 3, (50, 70))
    x = _x(37, 70, 8)
    bias = gen("normal_f32", 5, (50,))
    rec = (x.float() @ torch.from_numpy(w).float().T).to(torch.bfloat16)
    a, *_ = emulation_sums([Chunk(x=x, recorded=rec)], w, FMTS, bias)
    b, *_ = emulation_sums([Chunk(x=x, recorded=rec)], w, FMTS, bias, x_format="bf16")
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("x_format", ["bfp8", "bfp4", "bfp2"])
def test_chunking_does_not_change_qx(x_format):
    w = gen("normal_f32", 3, (40, 48))
    x = _x(23, 48, 9)
    whole = quantize_x(x, x_format).numpy()
    one, *_ = emulation_sums([Chunk(x=x)], w, FMTS, None, x_format=x_format)
    for size in (1, 3, 23):
        parts = [x[s: s + size] for s in range(0, 23, size)]
        assert np.array_equal(np.concatenate([quantize_x(p, x_format).numpy() for p in parts]), whole)
        got, *_ = emulation_sums([Chunk(x=p) for p in parts], w, FMTS, None, x_format=x_format)
        np.testing.assert_allclose(got, one, rtol=1e-13, atol=1e-13 * np.abs(one).max())


@pytest.mark.parametrize("bad", ["mxfp4", "nvfp4", "fp0", "x"])
def test_non_activation_formats_are_refused(bad):
    w = gen("normal_f32", 3, (8, 16))
    x = _x(4, 16, 1)
    with pytest.raises(ValueError, match="activation format"):
        emulation_sums([Chunk(x=x)], w, FMTS, x_format=bad)
    with pytest.raises(ValueError, match="activation format"):
        hip_sums([Chunk(x=x)], w, FMTS, x_format=bad)
    with pytest.raises(ValueError, match="activation format"):
        quantize_x(x, bad)
    with pytest.raises(ValueError, match="activation format"):
        hb.quantize_rows_bf16(x, bad)


def test_evaluate_op_refuses_and_records_the_x_format(tmp_path):
    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "up_proj", "all")
    with pytest.raises(ValueError, match="activation format"):
        evaluate_op(index, ops[0], ["bf16"], x_format="nvfp4")
    assert evaluate_op(index, ops[0], ["bf16"], x_format="bfp2").x_format == "bfp2"
    assert evaluate_op(index, ops[0], ["bf16"]).x_format == "bf16"


def test_c_entry_points_check_arguments():
    L = hb.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    sz = L.mtq_output_error_scratch_doubles(4, 50)
    qx = L.mtq_output_error_qx
    assert qx(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, None, 40) == -1
    assert b"xq is null" in L.mtq_last_error()
    assert qx(None, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, p, 40) == -1
    assert b"null" in L.mtq_last_error()
    assert qx(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, p, 39) == -1
    assert b"ldxq < k" in L.mtq_last_error()
    assert qx(p, 4, 40, 40, p, 0, 50, 40, None, 0x1F, None, None, 0, 0, p, p, sz, None, p, 40) == -4   # format bit 4
    assert qx(p, 4, 40, 40, p, 7, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, p, 40) == -1    # w dtype
    assert qx(p, 4, 40, 39, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None, p, 40) == -1
    assert b"ldx < k" in L.mtq_last_error()
    assert qx(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, 1, None, p, 40) == -1
    assert b"scratch" in L.mtq_last_error()
    rows = L.mtq_quantize_rows_bf16
    assert rows(None, 4, 40, 40, 1, p, 40, None) == -1 and b"null" in L.mtq_last_error()
    assert rows(p, 4, 40, 40, 1, None, 40, None) == -1 and b"null" in L.mtq_last_error()
    for fmt in (hb.FMT_CODE["fp0"], hb.QUANTIZE_CODE["mxfp4"], hb.QUANTIZE_CODE["nvfp4"], -1, 9):
        assert rows(p, 4, 40, 40, fmt, p, 40, None) == -4, fmt
        assert b"activation format" in L.mtq_last_error()
    assert rows(p, 4, 40, 39, 1, p, 40, None) == -1 and b"ld < cols" in L.mtq_last_error()
    assert rows(p, 4, 40, 40, 1, p, 39, None) == -1 and b"ldy < cols" in L.mtq_last_error()
    assert rows(p, 0, 40, 40, 1, p, 40, None) == -1


def _cli(model, io, out, *extra):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0.mlp",
                        "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--compression-config",
                        str(ROOT / "compression_configs" / "greedy_seed123.json"), "--out-dir", str(out), *extra],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, json.loads((out / "layer_output_error.json").read_text()), (out / "layer_output_error.csv").read_text()


def test_cli_x_format_end_to_end(tmp_path):
    model, io = make_fixture(tmp_path)
    out_q, doc_q, csv_q = _cli(model, io, tmp_path / "q", "--x-format", "bfp4")
    out_p, doc_p, csv_p = _cli(model, io, tmp_path / "p")
    out_b, doc_b, csv_b = _cli(model, io, tmp_path / "b", "--x-format", "bf16")
    assert doc_q["x_format"] == "bfp4" and doc_p["x_format"] == "bf16"
    assert "W 30x70  X bfp4  M 12" in out_q and "W 50x40  X bfp4  M 26" in out_q and "  X " not in out_p
    # without the flag: the output of an explicit bf16 run, the columns of the CSV as before
    assert csv_p == csv_b and out_p.replace(str(tmp_path / "p"), "") == out_b.replace(str(tmp_path / "b"), "")
    assert next(csv.reader(csv_p.splitlines())) == ["op", "candidate", "bytes", "pcc", "mae", "atol", "M", "N", "K"]
    assert csv_q.count("\n") == csv_p.count("\n") == 1 + 2 * 7
    for oq, op in zip(doc_q["ops"], doc_p["ops"]):
        assert oq["op"] == op["op"] and oq["M"] == op["M"]
        rq, rp = {r["candidate"]: r for r in oq["rows"]}, {r["candidate"]: r for r in op["rows"]}
        assert list(rq) == list(rp)
        for name in rq:
            if name in ("recorded", "fp0"):
                assert rq[name] == rp[name], (oq["op"], name)
            else:
                assert rq[name]["bytes"] == rp[name]["bytes"]
                assert rq[name]["pcc"] != rp[name]["pcc"] and rq[name]["mae"] > rp[name]["mae"], (oq["op"], name, rq[name], rp[name])
    # the rows without the flag are the emulation of X as recorded
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp", "all")
    for op, rec in zip(ops, doc_p["ops"]):
        res = evaluate_op(index, op, ["bf16", "bfp8", "bfp4", "bfp2", "fp0"])
        for row in res.rows:
            want = {r["candidate"]: r for r in rec["rows"]}[row.candidate]
            assert (row.pcc, row.mae, row.atol) == (want["pcc"], want["mae"], want["atol"])
