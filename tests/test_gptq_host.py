"""GPTQ on the host: the fixed-exponent element rule against quantize_weight_values, the sweep's identities (diagonal H gives RTN, grid
membership, bf16 exactness, Σ loss = Σ δ H_d δᵀ), its gain on correlated activations, the CLI's GPTQ rows and the new C entry points'
argument checks."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import emulation_sums
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.test_budget_maps_host import loe_sse, quality_case
from tests.test_output_error_host import make_fixture

ROOT = Path(__file__).resolve().parent.parent
ALL = list(MIXED_TILE_FORMATS)


def signed_zero_equal(a, b) -> bool:
    """Bitwise equality with −0 == +0 (a −0 weight may come back +0 from −0 − (−0) in the sweep's updates)."""
    a = np.asarray(a, dtype=np.float32) + np.float32(0.0)
    b = np.asarray(b, dtype=np.float32) + np.float32(0.0)
    return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def correlated_case(seed: int, n: int = 128, k: int = 256, tokens: int = 2048):
    """W n × k ~ N(0, 0.02); X = Z·A with a fixed-seed k × k mixing A (Z ~ N(0, 1)); calibration and evaluation drawn separately."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.02
    a = torch.randn(k, k, generator=g) / np.sqrt(k)

    def acts():
        return (torch.randn(tokens, k, generator=g) @ a).to(torch.bfloat16)

    return w, acts(), acts()


def _special_values(rng, rows: int, k: int) -> np.ndarray:
    x = (rng.standard_normal((rows, k)) * 0.05).astype(np.float32)
    x[0, :16] = 0.0                                               # an all-zero group
    x[1, :16] = np.float32(2.0 ** -130) * np.arange(16)           # subnormals only
    x[2, 16:32] *= np.float32(2.0 ** -120)                        # subnormals next to normals
    x[2, 20] = np.float32(2.0 ** -125)
    x[3, :16] = [1.0, 0.375, 0.125, -0.625, 0.875, 0.0625, -0.1875, 0.3125, 0.5, 0.75, -0.25, 0.9375, 0.0, -0.0, 0.4375, 0.5625]   # ties
    x[4, :16] = np.float32(3.4028235e38) * np.sign(rng.standard_normal(16)).astype(np.float32)  # ±max
    x[5, 32:48] = -np.float32(1.5)
    return x


@pytest.mark.parametrize("fmt", ALL)
def test_fixed_exponent_rule_with_own_exponent_is_quantize_weight_values(fmt):
    rng = np.random.default_rng(ALL.index(fmt))
    x = _special_values(rng, 12, 80)
    g = x.reshape(12, 5, 16)
    E = gq.group_exponent(g)[..., None]
    got = gq.q_fixed(g, ALL.index(fmt), E).reshape(x.shape)
    want = quantize_weight_values(x, fmt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # float64 input: rounded to float32 first
    x64 = x.astype(np.float64) * (1 + 2.0 ** -40)
    got64 = gq.q_fixed(x64.reshape(12, 5, 16), ALL.index(fmt), gq.group_exponent(x64.astype(np.float32).reshape(12, 5, 16))[..., None])
    assert np.array_equal(got64.reshape(x.shape).view(np.uint32), quantize_weight_values(x64.astype(np.float32), fmt).view(np.uint32))


@pytest.mark.parametrize("code,m", [(1, 7), (2, 3), (3, 1)])
def test_exponent_above_E_saturates_with_its_sign(code, m):
    E = 127                                                       # step = 2^(1 − m): the largest level (2^m − 1)·step < 2
    step = 2.0 ** (E - 126 - m)
    x = np.array([2.0, -2.0, 3.0e5, -7.5, 1.0, -1.0], dtype=np.float32)
    got = gq.q_fixed(x, code, E)
    top = (2 ** m - 1) * step
    assert got[:4].tolist() == [top, -top, top, -top]
    assert got[4:].tolist() == quantize_weight_values(np.array([1.0, -1.0] + [0.5] * 14, np.float32), ALL[code])[:2].tolist()
    # the unchanged helper returns 0 there (the d > 31 wrap); with E the group's own maximum they agree
    assert np.array_equal(gq.bfp_fixed_bits(np.array([0x3F800000], np.uint32), 127, m), quantize_weight_values(np.float32([1.0]), ALL[code]).view(np.uint32))


def _diag_u(k, rng):
    return gq.factor(np.diag(rng.random(k) + 0.5))


@pytest.mark.parametrize("n,k,wdt", [(70, 100, "f32"), (33, 40, "bf16"), (64, 64, "f32")])
def test_diagonal_hessian_gives_rtn(n, k, wdt):
    rng = np.random.default_rng(n * k)
    w = _special_values(rng, n, k)
    w[4, :] = rng.standard_normal(k).astype(np.float32)           # no ±max rows: they stay finite but RTN keeps them
    w[7, 3] = -0.0
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32)
    w32 = wt.float().numpy()
    u = _diag_u(k, rng)
    for f in ALL:
        q, loss, _ = gq.sweep_emulation(wt, u, gq.constant_codes(n, k, f))
        assert signed_zero_equal(q, quantize_weight_values(w32, f)), f
        assert np.all(np.isfinite(loss))
    a = rng.integers(0, 4, size=bm.tiles_hw(n, k)).astype(np.int8)
    q, _loss, _ = gq.sweep_emulation(wt, u, a)
    assert signed_zero_equal(q, bm.reconstruct_emulation(w32, a))


@pytest.mark.parametrize("seed", range(3))
def test_grid_membership_bf16_exactness_and_loss_identity(seed):
    w, x_cal, _ = correlated_case(seed, n=70, k=100, tokens=500)
    h, m = gq.gram_full_emulation([Chunk(x=x_cal[:200]), Chunk(x=x_cal[200:])], 100)
    assert m == 500 and np.array_equal(h, h.T)
    u = gq.factor(h)
    hd = gq.damped_hessian(h)
    rng = np.random.default_rng(seed)
    for codes in [gq.constant_codes(70, 100, f) for f in ALL] + [rng.integers(0, 4, size=(3, 4)).astype(np.int8)]:
        q, loss, margin = gq.sweep_emulation(w, u, codes)
        assert np.array_equal(bm.reconstruct_emulation(q, codes).view(np.uint32), q.view(np.uint32))
        if (codes == codes.flat[0]).all():
            f = ALL[int(codes.flat[0])]
            assert np.array_equal(quantize_weight_values(q, f).view(np.uint32), q.view(np.uint32))
        assert np.array_equal(torch.from_numpy(q).to(torch.bfloat16).float().numpy().view(np.uint32), q.view(np.uint32))
        want = gq.quadratic_loss(w, q, hd)
        assert abs(loss.sum() - want.sum()) <= 1e-9 * want.sum()
        assert np.all(np.abs(loss - want) <= 1e-9 * want + 1e-300)
        assert margin.shape == (70,) and np.all(margin >= 0)


def test_factor_reasons_and_dead_columns():
    with pytest.raises(ValueError):
        gq.factor(np.eye(4), 0.0)
    with pytest.raises(ValueError):
        gq.factor(np.eye(4), float("nan"))
    h = np.zeros((4, 4))
    h[0, 0] = 2.0
    hd = gq.damped_hessian(h, 0.5)
    assert np.allclose(np.diag(hd), [2.0 + 0.625, 1.625, 1.625, 1.625])
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])                      # indefinite: damping 1 % does not rescue it
    assert isinstance(gq.factor(bad), str)
    assert isinstance(gq.factor(np.array([[np.inf, 0.0], [0.0, 1.0]])), str)
    # a dead column is rounded like RTN (W is not zeroed)
    x = torch.zeros((50, 32), dtype=torch.bfloat16)
    x[:, :16] = torch.randn(50, 16).to(torch.bfloat16)
    h, _ = gq.gram_full_emulation([Chunk(x=x)], 32)
    w = torch.randn(8, 32) * 0.05
    q, _, _ = gq.sweep_emulation(w, gq.factor(h), gq.constant_codes(8, 32, "bfp4"))
    assert np.array_equal(q[:, 16:], quantize_weight_values(w.numpy(), "bfp4")[:, 16:])


def _gain(w, x_cal, x_eval, fmt):
    k = int(w.shape[1])
    h, _ = gq.gram_full_emulation([Chunk(x=x_cal)], k)
    hd = gq.damped_hessian(h)
    codes = gq.constant_codes(int(w.shape[0]), k, fmt)
    q, loss, _ = gq.sweep_emulation(w, gq.factor(h), codes)
    rtn = quantize_weight_values(w.numpy(), fmt)
    sse_g, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, q)
    sse_r, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, rtn)
    return loss.sum() / gq.quadratic_loss(w, rtn, hd).sum(), loe_sse(sse_g[4]) / loe_sse(sse_r[4])


def test_gptq_beats_rtn_on_mixed_activations():
    """X = Z·A: measured on the emulation, GPTQ's calibration loss / RTN's δH_dδᵀ is 0.52 (bfp4) and 0.68 (bfp2), the held-out LOE SSE
    ratio 0.55 and 0.72 (bfp8: 0.49 / 0.51).  Pinned with margin."""
    w, x_cal, x_eval = correlated_case(1)
    for fmt, limit in (("bfp4", 0.65), ("bfp2", 0.8)):
        cal_ratio, eval_ratio = _gain(w, x_cal, x_eval, fmt)
        assert cal_ratio < limit and eval_ratio < limit, (fmt, cal_ratio, eval_ratio)


def test_gptq_on_outlier_channels_wins_calibration_loss_only():
    """quality_case (i.i.d. channels, two ×30 outliers) has a nearly diagonal H: there is little to compensate.  Measured at 4096
    tokens: calibration loss ratio 0.957 (bfp4) and 0.964 (bfp2), but the held-out LOE SSE ratio is 1.046 for both (1.009 / 1.013 at
    16384 tokens): the sweep fits the sample Hessian's off-diagonal noise.  Pinned: the calibration gain, and held-out within 10 %."""
    w, x_cal, x_eval = quality_case(1)
    for fmt in ("bfp4", "bfp2"):
        cal_ratio, eval_ratio = _gain(w, x_cal, x_eval, fmt)
        assert cal_ratio < 0.99 and eval_ratio < 1.1, (fmt, cal_ratio, eval_ratio)


def _run(args, cwd=ROOT):
    return subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), *args], capture_output=True, text=True,
                          cwd=cwd, timeout=600)


def test_cli_gptq_rows(tmp_path):
    model, io = make_fixture(tmp_path)
    base = [str(model), str(io), "model.layers.0.mlp", "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--split", "test",
            "--compression-config", str(ROOT / "compression_configs" / "compression_config.mixed_tile_greedy.example.json")]
    r0 = _run(base + ["--out-dir", str(tmp_path / "plain")])
    r1 = _run(base + ["--out-dir", str(tmp_path / "gptq"), "--gptq", "--budget-bits", "4"])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    d0 = json.loads((tmp_path / "plain" / "layer_output_error.json").read_text())
    d1 = json.loads((tmp_path / "gptq" / "layer_output_error.json").read_text())
    assert "gptq_damp" not in d0 and d1["gptq_damp"] == 0.01 and d1["calib_split"] == "calibration"
    for o0, o1 in zip(d0["ops"], d1["ops"]):
        rows = {x["candidate"]: x for x in o1["rows"]}
        assert o1["rows"][: len(o0["rows"])] == o0["rows"]
        extra = [x["candidate"] for x in o1["rows"][len(o0["rows"]):]]
        map_name = next(x["candidate"] for x in o0["rows"] if x["candidate"].startswith("map:"))
        assert extra == ["budget:4:output", "budget:4:weight", "gptq:bfp8", "gptq:bfp4", "gptq:bfp2", f"gptq:{map_name}",
                         "gptq:budget:4:output"], extra
        for name in extra[2:]:
            x = rows[name]
            assert x["bytes"] == rows[name[len("gptq:"):]]["bytes"]
            assert x["damp"] == 0.01 and x["calib_tokens"] > 0 and x["calib_loss"] >= 0.0 and 0.0 < x["pcc"] <= 1.0
        assert o1["budget_skipped"] == []
    # without --budget-bits: the GPTQ rows alone, and the calibration keys
    r2 = _run(base + ["--out-dir", str(tmp_path / "g2"), "--gptq", "--gptq-damp", "0.1"])
    assert r2.returncode == 0, r2.stderr
    d2 = json.loads((tmp_path / "g2" / "layer_output_error.json").read_text())
    assert "budget_bits" not in d2 and d2["gptq_damp"] == 0.1
    assert [x["candidate"] for x in d2["ops"][0]["rows"]][-4:][0] == "gptq:bfp8"
    assert all(x["damp"] == 0.1 for x in d2["ops"][0]["rows"] if x["candidate"].startswith("gptq:"))


def test_cli_gptq_without_calibration_tokens_and_argument_errors(tmp_path):
    model, io = make_fixture(tmp_path, n_cal=0, n_test=2)
    r = _run([str(model), str(io), "model.layers.0.mlp.up_proj", "--split", "test", "-c", "bfp4", "bfp2", "--gptq",
              "--out-dir", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    up = json.loads((tmp_path / "o" / "layer_output_error.json").read_text())["ops"][0]
    assert not any(x["candidate"].startswith("gptq:") for x in up["rows"])
    assert [x["candidate"] for x in up["budget_skipped"]] == ["gptq:bfp4", "gptq:bfp2"]
    assert "no calibration samples" in up["budget_skipped"][0]["reason"] and "gptq:bfp4" in r.stdout
    for bad, flag in ((["--gptq", "--x-format", "bfp8"], "--gptq"), (["--gptq", "--gptq-damp", "0"], "--gptq-damp"),
                      (["--gptq", "--gptq-damp", "-1"], "--gptq-damp"), (["--gptq", "--gptq-damp", "nan"], "--gptq-damp")):
        r = _run([str(model), str(io), "up_proj", *bad, "--out-dir", str(tmp_path / "e")])
        assert r.returncode == 2 and flag in r.stderr, (bad, r.stderr)


def test_evaluate_op_without_calibration_gives_reasons(tmp_path):
    from quantization_analysis_amd.layer_io import select_ops
    from quantization_analysis_amd.model_source import build_model_index
    from quantization_analysis_amd.output_error import evaluate_op

    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp.down_proj", "test")
    res = evaluate_op(index, ops[0], ["bfp8", "bfp4"], None, "emulation", calib=None, gptq=True)
    assert [c for c, _ in res.budget_skipped] == ["gptq:bfp8", "gptq:bfp4"] and "no calibration samples" in res.budget_skipped[0][1]
    assert [r.candidate for r in res.rows] == ["bfp8", "bfp4", "recorded"]
    res = evaluate_op(index, ops[0], ["bf16", "fp0"], None, "emulation", calib=None, gptq=True)
    assert res.budget_skipped == []                              # no BFP format, no map: no GPTQ candidate
    with pytest.raises(ValueError):
        evaluate_op(index, ops[0], ["bfp4"], None, "emulation", x_format="bfp4", calib=None, gptq=True)
    with pytest.raises(ValueError):
        evaluate_op(index, ops[0], ["bfp4"], None, "emulation", calib=None, gptq=True, gptq_damp=0.0)


def test_c_entry_points_check_arguments():
    L = hb.lib()
    buf = np.zeros(1 << 14, dtype=np.float64)
    p = buf.ctypes.data
    assert L.mtq_gram_full_scratch_doubles(0, 32) == 0 and L.mtq_gram_full_scratch_doubles(16384, 7168) == 0
    sz = L.mtq_gram_full_scratch_doubles(1000, 40)
    assert sz > 0 and sz % (16 * 1024) == 0
    ok = (p, 1000, 40, 40, p, 1600, p, sz, None)

    def gram(**kw):
        args = dict(zip(("x", "m", "k", "ldx", "h", "hd", "s", "sd", "st"), ok))
        args.update(kw)
        return L.mtq_gram_full(*args.values())

    assert gram(x=None) == -1 and b"null" in L.mtq_last_error()
    assert gram(h=None) == -1 and gram(s=None) == -1
    assert gram(ldx=39) == -1 and b"ldx < k" in L.mtq_last_error()
    assert gram(hd=1601) == -1 and b"h_doubles" in L.mtq_last_error()
    assert gram(sd=sz - 1) == -1 and b"scratch" in L.mtq_last_error()
    assert gram(m=0) == -1
    assert L.mtq_gptq_sweep_scratch_doubles(70, 100) == 96 * 128 and L.mtq_gptq_sweep_scratch_doubles(0, 5) == 0
    oks = (p, 1, 50, 40, 40, p, 1600, p, 4, p, 40, p, p, 64 * 64, None)

    def sweep(**kw):
        args = dict(zip(("w", "dt", "n", "k", "ldw", "u", "ud", "c", "cc", "o", "ldo", "l", "s", "sd", "st"), oks))
        args.update(kw)
        return L.mtq_gptq_sweep(*args.values())

    for key in ("w", "u", "c", "o", "l", "s"):
        assert sweep(**{key: None}) == -1 and b"null" in L.mtq_last_error()
    assert sweep(dt=5) == -1 and b"w_dtype" in L.mtq_last_error()
    assert sweep(ldw=39) == -1 and b"ldw < k" in L.mtq_last_error()
    assert sweep(ldo=39) == -1 and b"ldo < k" in L.mtq_last_error()
    assert sweep(ud=1599) == -1 and b"u_doubles" in L.mtq_last_error()
    assert sweep(cc=3) == -1 and b"code_count" in L.mtq_last_error()
    assert sweep(sd=64 * 64 - 1) == -1 and b"scratch" in L.mtq_last_error()
    assert sweep(s=p + 8) == -1 and b"aligned" in L.mtq_last_error()
    assert sweep(n=0) == -1


def test_python_wrappers_check_arguments():
    x = torch.zeros((4, 40), dtype=torch.bfloat16)
    h = torch.zeros((40, 40), dtype=torch.float64)
    with pytest.raises(hb.MtqError):
        hb.gram_full(x, h)                                      # host tensors
    with pytest.raises(hb.MtqError):
        hb.gram_full(x.float(), h)
    with pytest.raises(hb.MtqError):
        hb.gram_full(x.t(), h)
    c = torch.zeros((1, 2), dtype=torch.int8)
    with pytest.raises(hb.MtqError):
        hb.gptq_sweep(torch.zeros((8, 40)), h, c)
    with pytest.raises(hb.MtqError):
        hb.gptq_sweep(torch.zeros((8, 40), dtype=torch.float16), h, c)
