"""GPTQ on the MI355X: the full Gram kernel against float64 within its contract's bound (symmetric, deterministic, chunked), the sweep
against the host emulation on the same host-factorised U (bitwise on rows whose decisions are clear), the diagonal-H case against
round-to-nearest, and the GPTQ rows of evaluate_op and the CLI.  The exact cases (integer X, dyadic W and U: bit equality on every
entry and every row, the rows on a tie and the saturating ones included) are in test_calibration_exact_gpu.py."""
from __future__ import annotations

import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import SLOTS, _gptq_outputs, emulation_sums, hip_sums
from tests.test_budget_maps_host import loe_sse
from tests.test_gptq_host import correlated_case, signed_zero_equal
from tests.test_output_error_gpu import _check, _eps
from tests.test_output_error_host import make_fixture

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ALL = list(MIXED_TILE_FORMATS)


@pytest.mark.parametrize("k", [32, 40, 7168])
@pytest.mark.parametrize("m,parts", [(1, 1), (17, 1), (1000, 1), (40000, 3)])
def test_gram_full_within_bound_symmetric_and_deterministic(k, m, parts):
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(m * 31 + k)
    off = 1 if m % 2 else 0                                     # odd offset: the element-wise staging path; else ldx = k + 8, aligned
    base = (torch.randn((m, k + 8), generator=g, device="cuda") * 3).to(torch.bfloat16)
    x = base[:, off: off + k]
    assert x.stride(0) == k + 8 > k
    cuts = np.linspace(0, m, parts + 1).astype(int)
    h = torch.zeros((k, k), dtype=torch.float64, device="cuda")
    h2 = torch.zeros_like(h)
    for a, b in zip(cuts[:-1], cuts[1:]):
        hb.gram_full(x[a:b], h)
        hb.gram_full(x[a:b], h2)
    xd = x.double()
    want = xd.T @ xd
    absx = xd.abs().T @ xd.abs()
    torch.cuda.synchronize()
    assert torch.equal(h, h2)
    assert torch.equal(h, h.T)
    err = (h - want).abs()
    assert bool((err <= 2.0 ** -15 * absx).all()), float((err / absx.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def _factor(k: int, tokens: int = 4096):
    """U of correlated activations (X = Z·A, fixed seed) for k columns, factorised on the host."""
    g = torch.Generator(device="cuda").manual_seed(k)
    a = torch.randn((k, k), generator=g, device="cuda", dtype=torch.float64) / np.sqrt(k)
    x = (torch.randn((tokens, k), generator=g, device="cuda", dtype=torch.float64) @ a).to(torch.bfloat16)
    xd = x.double()
    h = (xd.T @ xd).cpu().numpy()
    u = gq.factor(h)
    assert not isinstance(u, str), u
    return u


def _codes(n, k, kind, seed):
    if kind == "map":
        return np.random.default_rng(seed).integers(0, 4, size=(-(-n // 32), -(-k // 32))).astype(np.int8)
    return gq.constant_codes(n, k, kind)


CASES = [(70, 100, "f32", "bfp4"), (70, 100, "bf16", "map"), (300, 200, "bf16", "bfp2"), (300, 200, "f32", "map"),
         (300, 200, "f32", "bfp8"), (64, 7168, "bf16", "map"), (64, 7168, "f32", "bfp4")]


@pytest.mark.parametrize("n,k,wdt,kind", CASES)
def test_sweep_matches_emulation_on_clear_rows(n, k, wdt, kind):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + k)
    w = (rng.standard_normal((n, k + 3)) * 0.05).astype(np.float32)
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32).cuda()[:, 1: 1 + k]   # ldw > k, offset
    codes = _codes(n, k, kind, n * k)
    u = _factor(k)
    what, loss = gq.sweep_hip(wt, u, codes)
    what2, loss2 = gq.sweep_hip(wt.contiguous(), u, codes)
    got = what.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), what2.cpu().numpy().view(np.uint32))
    assert torch.equal(loss, loss2)
    want, want_loss, margin = gq.sweep_emulation(wt.cpu(), u, codes)
    clear = margin > 2.0 ** -20
    # an element is unclear with probability ≈ 2·2⁻²⁰ (its value uniform within its step): ≈ 1.4 % of the rows at k = 7168 (measured:
    # 63 of 64 rows clear), below 0.1 % at k ≤ 300
    assert clear.mean() >= (0.99 if k <= 1024 else 0.95), clear.mean()
    assert np.array_equal(got[clear].view(np.uint32), want[clear].view(np.uint32)), np.nonzero((got != want).any(axis=1) & clear)
    lh = loss.cpu().numpy()
    assert np.all(np.abs(lh[clear] - want_loss[clear]) <= 1e-9 * want_loss[clear] + 1e-300)
    # grid membership and bf16 exactness of the device output
    assert np.array_equal(got.view(np.uint32), torch.from_numpy(got).to(torch.bfloat16).float().numpy().view(np.uint32))
    from quantization_analysis_amd.budget_maps import reconstruct_emulation

    assert np.array_equal(reconstruct_emulation(got, codes).view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("n,k,wdt", [(70, 100, "f32"), (300, 200, "bf16")])
def test_diagonal_hessian_gives_round_to_nearest(n, k, wdt):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(k)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[3, :16] = 0.0
    w[4, 5] = -0.0
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32).cuda()
    u = gq.factor(np.diag(rng.random(k) + 0.5))
    for kind in ("bfp8", "bfp4", "bfp2", "map"):
        codes = _codes(n, k, kind, 7)
        what, _loss = gq.sweep_hip(wt, u, codes)
        want = hb.apply_assignment(wt, codes) if kind == "map" else hb.quantize(wt, kind)
        assert signed_zero_equal(what.cpu().numpy(), want.cpu().numpy()), kind
        if kind != "map":
            assert torch.equal(hb.quantize(what, kind), what)


def test_evaluate_op_gptq_rows_on_hip(tmp_path):
    torch.cuda.set_device(0)
    from quantization_analysis_amd.layer_io import chunks, select_ops
    from quantization_analysis_amd.model_source import build_model_index
    from quantization_analysis_amd.output_error import evaluate_op

    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp", "test")
    cal, _ = select_ops(index, io, "model.layers.0.mlp", "calibration")
    cal = {o.op: o for o in cal}
    for op in ops:
        fm = ["bf16", "bfp8", "bfp4", "bfp2"]
        rh = evaluate_op(index, op, fm, None, "hip", budgets=(4.0,), calib=cal[op.op], gptq=True)
        re_ = evaluate_op(index, op, fm, None, "emulation", budgets=(4.0,), calib=cal[op.op], gptq=True)
        names = [r.candidate for r in rh.rows]
        assert names[-4:] == ["gptq:bfp8", "gptq:bfp4", "gptq:bfp2", "gptq:budget:4:output"], names
        assert [r.candidate for r in re_.rows] == names and rh.budget_skipped == []
        for a, b in zip(rh.rows[-4:], re_.rows[-4:]):
            assert a.bytes == b.bytes and a.extra["calib_tokens"] == b.extra["calib_tokens"] > 0
            assert abs(a.extra["calib_loss"] - b.extra["calib_loss"]) <= 0.05 * b.extra["calib_loss"] + 1e-12, (a.candidate, a.extra, b.extra)
            assert abs(loe_sse(a.sums) - loe_sse(b.sums)) <= 0.05 * loe_sse(b.sums) + 1e-12, (a.candidate, a.sums, b.sums)


def test_hip_rows_equal_emulation_of_the_hip_weights():
    """The hip route evaluates its own Ŵ exactly (through the bf16 slot): its sums against emulation_sums of that Ŵ, within the LOE
    kernel's f32 bound; the held-out SSE of every GPTQ candidate within a few percent of the all-emulation run's."""
    torch.cuda.set_device(0)
    w, x_cal, x_eval = correlated_case(3, n=256, k=256)
    hd_dev, m = gq.gram_full_hip([Chunk(x=x_cal)], 256)
    u_hip = gq.factor(hd_dev.cpu().numpy())
    h_emu, _ = gq.gram_full_emulation([Chunk(x=x_cal)], 256)
    u_emu = gq.factor(h_emu)
    for f in ("bfp8", "bfp4", "bfp2"):
        codes = gq.constant_codes(256, 256, f)
        what, _loss = gq.sweep_hip(w.cuda(), u_hip, codes)
        got, *_ = hip_sums(_gptq_outputs([Chunk(x=x_eval)], what, None), w, [], None)
        y = what.cpu().numpy()
        want, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, y)
        xf = x_eval.float().numpy()
        _check(got[SLOTS.index("recorded")], want[SLOTS.index("map")], float(x_eval.shape[0] * 256), _eps(xf, [w.numpy()], None, 256),
               _eps(xf, [y], None, 256), f)
        y_emu, _l, _mg = gq.sweep_emulation(w, u_emu, codes)
        ref, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, y_emu)
        s_hip, s_emu = loe_sse(want[SLOTS.index("map")]), loe_sse(ref[SLOTS.index("map")])
        assert abs(s_hip - s_emu) <= 0.02 * s_emu, (f, s_hip, s_emu)    # measured: equal (no row of Ŵ differs here)


def test_cli_gptq_on_hip_agrees_with_emulation(tmp_path):
    model, io = make_fixture(tmp_path)
    docs = {}
    for backend in ("emulation", "hip"):
        out = tmp_path / backend
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0.mlp",
                            "--backend", backend, "-c", "bf16", "bfp8", "bfp4", "bfp2", "--split", "test", "--gptq", "--out-dir", str(out)],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        docs[backend] = json.loads((out / "layer_output_error.json").read_text())
    for oe, oh in zip(docs["emulation"]["ops"], docs["hip"]["ops"]):
        assert [x["candidate"] for x in oe["rows"]] == [x["candidate"] for x in oh["rows"]]
        for re_, rh in zip(oe["rows"], oh["rows"]):
            assert re_["bytes"] == rh["bytes"]
            if re_["candidate"].startswith("gptq:"):
                assert rh["calib_tokens"] == re_["calib_tokens"] and rh["damp"] == re_["damp"] == 0.01
                assert abs(rh["calib_loss"] - re_["calib_loss"]) <= 0.05 * re_["calib_loss"] + 1e-12
            assert abs(re_["pcc"] - rh["pcc"]) < 1e-5, (oe["op"], re_, rh)
