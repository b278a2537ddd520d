"""Layer-output error on the MI355X: the fused kernel's sums against the float64 emulation within the bounds of f32
accumulation (DESIGN.md §LOE numerics), the map candidate against the unfused route (K3 y, then a float64 matmul), determinism,
chunking and the CLI."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.config import CompressionConfig
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import SLOTS, emulation_sums, hip_sums, search_map
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen
from tests.test_output_error_host import make_fixture

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FMTS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
U = 2.0 ** -24


def _eps(x, w_list, bias, k):
    """Per-output error bound of one f32-accumulated candidate: (K + 2)·2⁻²⁴·(1 + 2⁻⁷)·max_(m,n) (Σ_k |x_mk·w_nk| + |b_n|), w over
    every weight the candidate's accumulators saw (DESIGN.md §LOE numerics)."""
    xa = np.abs(np.asarray(x, dtype=np.float64))
    s = 0.0
    for w in w_list:
        t = xa @ np.abs(np.asarray(w, dtype=np.float64)).T
        if bias is not None:
            t = t + np.abs(np.asarray(bias, dtype=np.float64))
        s = max(s, float(t.max()) if t.size else 0.0)
    return (k + 2) * U * (1 + 2.0 ** -7) * s


def _check(got, want, count, eps_r, eps_q, what=""):
    """mae / atol within 2ε (+ the float64 summation term); pcc within 2ε_r/σ_r + 2ε_q/σ_q (+ the float64 moment term)."""
    g = hb.columns_from_sums(got, count)
    e = hb.columns_from_sums(want, count)
    f64 = 64 * count * 2.0 ** -53
    d_abs = eps_r + eps_q
    assert abs(g["mae"] - e["mae"]) <= d_abs + f64 * abs(e["mae"]) + 1e-300, (what, g, e)
    assert abs(g["atol"] - e["atol"]) <= d_abs + 2.0 ** -52 * abs(e["atol"]) + 1e-300, (what, g, e)
    n = count
    mr, mq = want[0] / n, want[2] / n
    vr, vq = max(want[1] / n - mr * mr, 0.0), max(want[3] / n - mq * mq, 0.0)
    sr, sq = np.sqrt(vr), np.sqrt(vq)
    if sr == 0.0 or sq == 0.0:
        assert g["pcc"] == e["pcc"], (what, g, e)
        return
    rms = np.sqrt(want[1] / n) * np.sqrt(max(want[3] / n, 0.0))
    bound = 2 * eps_r / sr + 2 * eps_q / sq + f64 * rms / (sr * sq)
    assert abs(g["pcc"] - e["pcc"]) <= bound, (what, g["pcc"], e["pcc"], bound)


SHAPES = [(37, 50, 40), (300, 130, 70), (129, 64, 200), (5, 1, 16), (64, 130, 33)]


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("kind", ["heavy_bf16", "heavy_f32", "normal_f32"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_kernel_sums_match_emulation(m, n, k, kind, with_bias):
    torch.cuda.set_device(0)
    seed = m * 7 + n * 13 + k
    w = gen(kind, seed, (n, k))
    x = torch.from_numpy(gen("normal_bf16", seed + 1, (m, k)) * 40).to(torch.bfloat16)
    bias = gen("normal_f32", seed + 2, (n,)) if with_bias else None
    rec = (x.float() @ torch.from_numpy(w).T + (0 if bias is None else torch.from_numpy(bias))) * 1.001
    rec = rec.to(torch.bfloat16)
    wt = torch.from_numpy(w).to(torch.bfloat16 if kind.endswith("bf16") else torch.float32)
    bt = None if bias is None else torch.from_numpy(bias)
    want, mm, seen, _ = emulation_sums([Chunk(x=x, recorded=rec)], wt, FMTS, bt)
    got, mg, seen_g, _ = hip_sums([Chunk(x=x, recorded=rec)], wt, FMTS, bt)
    assert mm == mg == m and seen and seen_g
    count = float(m * n)
    wf = wt.float().numpy()
    xf = x.float().numpy()
    eps_r = _eps(xf, [wf], bias, k)
    for f in FMTS:
        wq = quantize_weight_values(wf, f)
        eps_q = 0.0 if f == "fp0" else _eps(xf, [wq], bias, k)
        _check(got[SLOTS.index(f)], want[SLOTS.index(f)], count, eps_r, eps_q, f)
    _check(got[SLOTS.index("recorded")], want[SLOTS.index("recorded")], count, eps_r, 0.0, "recorded")


def test_unaligned_and_strided_operands():
    """ld ≠ K and odd offsets take the element-wise staging path; the sums equal those of contiguous copies bit for bit."""
    torch.cuda.set_device(0)
    m, n, k = 70, 45, 37
    xb = torch.from_numpy(gen("normal_bf16", 1, (m, k + 3))).to(torch.bfloat16).cuda()[:, 1: k + 1]
    wb = torch.from_numpy(gen("heavy_f32", 2, (n, k + 5))).cuda()[:, 3: k + 3]
    a = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
    b = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
    hb.output_error(xb, wb, 0xF, a)
    hb.output_error(xb.contiguous(), wb.contiguous(), 0xF, b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("algorithm,params", [("mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": 123}),
                                              ("mixed-tile-threshold", {"metric": "pcc", "threshold": 0.995})])
@pytest.mark.parametrize("kind", ["heavy_bf16", "normal_f32"])
def test_map_candidate_matches_unfused_route(algorithm, params, kind):
    """The map of a hip search: the kernel's map sums against K3's y (the search's reconstruction) through a float64 matmul."""
    torch.cuda.set_device(0)
    n, k, m = 96, 160, 150
    w = gen(kind, 11, (n, k))
    wt = torch.from_numpy(w).to(torch.bfloat16 if kind.endswith("bf16") else torch.float32)
    x = torch.from_numpy(gen("normal_bf16", 12, (m, k)) * 30).to(torch.bfloat16)
    cfg = CompressionConfig(algorithm=algorithm, params=params, quantization_formats=["bf16", "bfp8", "bfp4", "bfp2"], seed=None, random_seed=False)
    mc = search_map(wt.cuda(), cfg, "hip")
    y = hb.apply_assignment(wt.cuda(), torch.from_numpy(mc.assignment).cuda()).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), mc.y.cpu().numpy().view(np.uint32))
    want, *_ = emulation_sums([Chunk(x=x)], wt, [], None, y)
    got, *_ = hip_sums([Chunk(x=x)], wt, [], None, mc.assignment)
    xf = x.float().numpy()
    _check(got[SLOTS.index("map")], want[SLOTS.index("map")], float(m * n), _eps(xf, [wt.float().numpy()], None, k), _eps(xf, [y], None, k))


def test_deterministic_and_chunked():
    torch.cuda.set_device(0)
    n, k, m = 130, 70, 1000
    w = torch.from_numpy(gen("heavy_f32", 21, (n, k)))
    bias = torch.from_numpy(gen("normal_f32", 22, (n,)))
    x = torch.from_numpy(gen("normal_bf16", 23, (m, k)) * 20).to(torch.bfloat16)
    one, *_ = hip_sums([Chunk(x=x)], w, FMTS, bias)
    two, *_ = hip_sums([Chunk(x=x)], w, FMTS, bias)
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    parts, *_ = hip_sums([Chunk(x=x[s: s + 130]) for s in range(0, m, 130)], w, FMTS, bias)
    for f in FMTS:   # every output is formed as in one chunk: only the float64 summation order differs
        _check(parts[SLOTS.index(f)], one[SLOTS.index(f)], float(m * n), 0.0, 0.0, f)


def test_cli_hip_agrees_with_emulation(tmp_path):
    model, io = make_fixture(tmp_path)
    docs = {}
    for backend in ("emulation", "hip"):
        out = tmp_path / backend
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0.mlp",
                            "--backend", backend, "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--compression-config",
                            str(ROOT / "compression_configs" / "greedy_seed123.json"), "--out-dir", str(out)],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        docs[backend] = json.loads((out / "layer_output_error.json").read_text())
    for oe, oh in zip(docs["emulation"]["ops"], docs["hip"]["ops"]):
        assert oe["op"] == oh["op"] and oe["M"] == oh["M"]
        for re_, rh in zip(oe["rows"], oh["rows"]):
            assert re_["candidate"] == rh["candidate"] and re_["bytes"] == rh["bytes"]
            assert abs(re_["pcc"] - rh["pcc"]) < 1e-5, (oe["op"], re_, rh)
            for key in ("mae", "atol"):
                assert abs(re_[key] - rh[key]) <= 1e-5 * max(1.0, abs(re_[key])), (oe["op"], re_, rh)
