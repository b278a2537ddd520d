"""Layer-output error on the host: the reader of the reference's IO layout, the float64 emulation route against a direct
computation, the C entry points' argument checks and the CLI with --backend emulation."""
from __future__ import annotations

import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.config import CompressionConfig
from quantization_analysis_amd.layer_io import Chunk, chunks, discover_ops, select_ops
from quantization_analysis_amd.model_source import build_model_index
from quantization_analysis_amd.output_error import SLOTS, check_layout, emulation_sums, evaluate_op, search_map
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen

ROOT = Path(__file__).resolve().parent.parent
FMTS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]


def _save(root: Path, op: str, split: str, idx: int, args, kwargs, output):
    d = root / op.replace(".", "/") / split
    d.mkdir(parents=True, exist_ok=True)
    torch.save({"args": args, "kwargs": kwargs, "output": output, "sample_idx": idx, "split": split}, d / f"sample_{idx:04d}.pt")


def make_fixture(tmp: Path, n_cal: int = 2, n_test: int = 2, seed: int = 0):
    """A tiny model (safetensors) and its IO directory in the reference's layout: a Linear with bias called positionally with a
    3-D input, a Linear called with kwargs only, a norm (1-D weight), a Linear whose input has the wrong K and one with a tuple output."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(seed)
    w_up = (torch.randn(50, 40, generator=g) * 0.05).to(torch.bfloat16)
    b_up = torch.randn(50, generator=g) * 0.01
    w_dn = torch.randn(30, 70, generator=g) * 0.05               # float32 weight
    w_norm = torch.ones(40)
    w_bad = torch.randn(20, 40, generator=g) * 0.05
    w_tup = torch.randn(20, 40, generator=g) * 0.05
    model = tmp / "model"
    model.mkdir()
    save_file({"model.layers.0.mlp.up_proj.weight": w_up, "model.layers.0.mlp.up_proj.bias": b_up,
               "model.layers.0.mlp.down_proj.weight": w_dn, "model.layers.0.input_layernorm.weight": w_norm,
               "model.layers.0.self_attn.bad.weight": w_bad, "model.layers.0.self_attn.tup.weight": w_tup}, str(model / "m.safetensors"))
    io = tmp / "io"
    for idx in range(n_cal + n_test):
        split = "calibration" if idx < n_cal else "test"
        x = torch.randn(1, 5 + idx, 40, generator=g).to(torch.bfloat16)
        y = (x.float() @ w_up.float().T + b_up).to(torch.bfloat16)
        _save(io, "model.layers.0.mlp.up_proj", split, idx, (x,), {}, y)
        x2 = torch.randn(1, 3, 70, generator=g).to(torch.bfloat16)
        _save(io, "model.layers.0.mlp.down_proj", split, idx, (), {"input": x2}, (x2.float() @ w_dn.T).to(torch.bfloat16))
        _save(io, "model.layers.0.input_layernorm", split, idx, (x,), {}, x)
        _save(io, "model.layers.0.self_attn.bad", split, idx, (torch.randn(1, 4, 33, generator=g).to(torch.bfloat16),), {}, torch.zeros(1, 4, 20))
        _save(io, "model.layers.0.self_attn.tup", split, idx, (x,), {}, (torch.zeros(1, 5, 20), None))
    return model, io


@pytest.fixture()
def fixture_dirs(tmp_path):
    return make_fixture(tmp_path)


def test_discovery_splits_and_max_samples(fixture_dirs):
    model, io = fixture_dirs
    ops = discover_ops(io)
    assert set(ops) == {"model.layers.0.mlp.up_proj", "model.layers.0.mlp.down_proj", "model.layers.0.input_layernorm",
                        "model.layers.0.self_attn.bad", "model.layers.0.self_attn.tup"}
    assert [(s, i) for s, i, _ in ops["model.layers.0.mlp.up_proj"]] == [("calibration", 0), ("calibration", 1), ("test", 2), ("test", 3)]
    index = build_model_index(str(model))
    sel, skipped = select_ops(index, io, "model.layers.0.mlp", "test")
    assert [o.op for o in sel] == ["model.layers.0.mlp.down_proj", "model.layers.0.mlp.up_proj"] and not skipped
    up = sel[1]
    assert up.bias == "model.layers.0.mlp.up_proj.bias" and sel[0].bias is None
    assert [i for _, i, _ in up.samples] == [2, 3] and up.splits == ["test"]
    sel, _ = select_ops(index, io, "up_proj", "all", max_samples=3)
    assert [i for _, i, _ in sel[0].samples] == [0, 1, 2]
    # 3-D args[0] flattened over its leading dims; a kwargs-only call read from kwargs
    xs = list(chunks(sel[0], 40, 50))
    assert [c.x.shape for c in xs] == [(5, 40), (6, 40), (7, 40)] and all(c.recorded.shape[1] == 50 for c in xs)
    down, _ = select_ops(index, io, "down_proj", "calibration")
    assert [c.x.shape for c in chunks(down[0], 70, 30)] == [(3, 70), (3, 70)]


def test_skip_reasons(fixture_dirs):
    model, io = fixture_dirs
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0", "all")
    reasons = {o.op: evaluate_op(index, o, ["bf16"]).skipped for o in ops}
    assert "not 2-D" in reasons["model.layers.0.input_layernorm"]
    assert "input last dim 33" in reasons["model.layers.0.self_attn.bad"]
    assert "tuple" in reasons["model.layers.0.self_attn.tup"]
    assert reasons["model.layers.0.mlp.up_proj"] is None and reasons["model.layers.0.mlp.down_proj"] is None


def _direct(x, w, bias, wq):
    """float64 sums of Y = x·wqᵀ + b against R = x·wᵀ + b, written out directly."""
    x64 = np.asarray(x, dtype=np.float64)
    r = x64 @ np.asarray(w, dtype=np.float64).T
    q = x64 @ np.asarray(wq, dtype=np.float64).T if wq is not None else np.zeros_like(r)
    if bias is not None:
        r = r + bias
        q = q + bias
    d = np.abs(r - q)
    return np.array([r.sum(), (r * r).sum(), q.sum(), (q * q).sum(), (r * q).sum(), d.sum(), d.max()])


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", ["heavy_bf16", "normal_f32"])
def test_emulation_matches_direct_float64(kind, with_bias):
    w = gen(kind, 3, (50, 70))
    x = torch.from_numpy(gen("normal_bf16", 4, (37, 70)) * 50).to(torch.bfloat16)
    bias = gen("normal_f32", 5, (50,)) if with_bias else None
    sums, m, rec, cast = emulation_sums([Chunk(x=x[:20]), Chunk(x=x[20:])], w, FMTS, bias)
    assert m == 37 and not rec and not cast
    xf = x.float().numpy()
    for f in FMTS:
        want = _direct(xf, w, bias, None if f == "fp0" else quantize_weight_values(w, f))
        np.testing.assert_allclose(sums[SLOTS.index(f)], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_map_candidate_is_the_search_reconstruction():
    w = gen("normal_f32", 7, (64, 96))
    x = torch.from_numpy(gen("normal_bf16", 8, (16, 96))).to(torch.bfloat16)
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"metric": "pcc", "threshold": 0.999, "seed": 123},
                            quantization_formats=["bf16", "bfp8", "bfp4", "bfp2"], seed=None, random_seed=False)
    mc = search_map(w, cfg, "emulation")
    assert mc.assignment.shape == (2, 3) and mc.tile_bytes > 0
    sums, *_ = emulation_sums([Chunk(x=x)], w, ["bf16"], None, mc.y)
    np.testing.assert_allclose(sums[SLOTS.index("map")], _direct(x.float().numpy(), w, None, mc.y), rtol=1e-12)


def test_zero_denominator_rule():
    """All-zero X: R = Y = 0 (zero variance, identical) → pcc 1 like the searches; with a bias R = Y = b, still identical."""
    w = gen("normal_f32", 9, (40, 48))
    x = torch.zeros((8, 48), dtype=torch.bfloat16)
    from quantization_analysis_amd.output_error import rows_from_sums

    sums, m, _, _ = emulation_sums([Chunk(x=x)], w, FMTS)
    rows = {r.candidate: r for r in rows_from_sums(sums, m, 40, 48, FMTS, None, False)}
    for f in FMTS:
        assert rows[f].pcc == 1.0 and rows[f].mae == 0.0 and rows[f].atol == 0.0
    xr = torch.from_numpy(gen("normal_bf16", 1, (8, 48))).to(torch.bfloat16)
    sums, m, _, _ = emulation_sums([Chunk(x=xr)], w, ["fp0"])
    assert rows_from_sums(sums, m, 40, 48, ["fp0"], None, False)[0].pcc == 0.0   # Y = 0 against a varying R


def test_transpose_layout_raises():
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"layout": "transpose"}, quantization_formats=None, seed=None, random_seed=False)
    with pytest.raises(ValueError, match="row layout"):
        check_layout(cfg)


def test_c_entry_points_check_arguments():
    L = hb.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    sz = L.mtq_output_error_scratch_doubles(300, 130)
    assert sz == 3 * 3 * 37
    assert L.mtq_output_error(None, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None) == -1
    assert b"null" in L.mtq_last_error()
    assert L.mtq_output_error(p, 4, 40, 40, p, 0, 50, 40, None, 0x1F, None, None, 0, 0, p, p, sz, None) == -4   # format bit 4
    assert L.mtq_output_error(p, 4, 40, 40, p, 7, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None) == -1   # w dtype
    assert L.mtq_output_error(p, 4, 40, 39, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, sz, None) == -1
    assert b"ldx < k" in L.mtq_last_error()
    assert L.mtq_output_error(p, 4, 40, 40, p, 0, 50, 32, None, 0xF, None, None, 0, 0, p, p, sz, None) == -1
    assert b"ldw < k" in L.mtq_last_error()
    assert L.mtq_output_error(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, p, 0, 49, p, p, sz, None) == -1
    assert b"ldr < n" in L.mtq_last_error()
    assert L.mtq_output_error(p, 4, 40, 40, p, 0, 50, 40, None, 0xF, None, None, 0, 0, p, p, 1, None) == -1
    assert b"scratch" in L.mtq_last_error()


def test_cli_emulation_end_to_end(fixture_dirs, tmp_path):
    model, io = fixture_dirs
    out = tmp_path / "out"
    cfg = ROOT / "compression_configs" / "greedy_seed123.json"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0",
                        "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--compression-config", str(cfg),
                        "--split", "test", "--max-samples", "1", "--out-dir", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "candidate" in r.stdout and "recorded" in r.stdout and "skipped:" in r.stdout
    doc = json.loads((out / "layer_output_error.json").read_text())
    ops = {o["op"]: o for o in doc["ops"]}
    up = ops["model.layers.0.mlp.up_proj"]
    assert up["M"] == 7 and up["splits"] == ["test"] and up["x_cast"] is False and up["shape"] == [50, 40]
    cands = [row["candidate"] for row in up["rows"]]
    assert cands[:5] == FMTS and cands[5].startswith("map:") and cands[6] == "recorded"
    rows = {row["candidate"]: row for row in up["rows"]}
    assert rows["bf16"]["pcc"] == 1.0 and rows["bf16"]["atol"] == 0.0   # bf16 W: the bf16 candidate is W itself
    assert rows["recorded"]["pcc"] > 0.999                                 # the recorded output belongs to these weights
    assert {s["op"] for s in doc["skipped"]} == {"model.layers.0.input_layernorm", "model.layers.0.self_attn.bad", "model.layers.0.self_attn.tup"}
    assert (out / "layer_output_error.csv").read_text().count("\n") == 1 + 2 * 7
