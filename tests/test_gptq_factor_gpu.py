"""mtq_gptq_factor on the MI355X: inputs on which no operation rounds against the analytic factor, bit for bit; the residual
max|U·H_d·Uᵀ − I| against the host route's; the status word on bad pivots; the device factor through the sweep and the CLI."""
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
from tests.test_gptq_gpu import _codes
from tests.test_gptq_host import correlated_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NB = hb.GPTQ_FACTOR_BLOCK
RESIDUAL_C = 2.0   # the smallest power of two at least twice the largest ratio measured on the MI355X, 0.940 (profiles/gptq_factor.txt)


@functools.lru_cache(maxsize=None)
def exact_case(k: int, zero_at: int = -1):
    """H_d = (DZ)(DZ)ᵀ and its factor U = Z⁻¹D⁻¹: Z = I + N with N strictly upper triangular, integer, nonzero only where
    lev(i) < lev(j), lev(i) = 5i mod 4 (so N⁴ = 0 and Z⁻¹ = I − N + N² − N³ in integers), D = diag(2^s): every intermediate of a blocked
    factorisation is an integer times a power of two far below 2⁵³.  zero_at: that entry of D is 0 (the pivot there is 0)."""
    rng = np.random.default_rng(1000 + k)
    lev = (5 * np.arange(k)) % 4
    i, j = np.indices((k, k))
    n = np.where((i < j) & (lev[i] < lev[j]) & (rng.random((k, k)) < 0.3), rng.integers(-2, 3, size=(k, k)), 0).astype(np.float64)
    d = 2.0 ** rng.integers(-6, 7, size=k)
    zinv = np.eye(k) - n + n @ n - n @ n @ n
    if zero_at >= 0:
        d[zero_at] = 0.0
    r = d[:, None] * (np.eye(k) + n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return r @ r.T, zinv / d[None, :]


def _factor_dev(hd: np.ndarray):
    u, status = hb.gptq_factor(torch.from_numpy(np.ascontiguousarray(hd)).cuda())
    return u.cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("k", [1, 33, NB, NB + 1, 3 * NB + 7, 520])
def test_exact_factor(k):
    torch.cuda.set_device(0)
    hd, want = exact_case(k)
    u, status = _factor_dev(hd)
    assert status == 0 and np.array_equal(u, want) and not np.tril(u, -1).any(), (status, np.argwhere(u != want)[:8])
    u2, status2 = _factor_dev(hd)
    assert status2 == 0 and np.array_equal(u2.view(np.uint64), u.view(np.uint64))


@functools.lru_cache(maxsize=None)
def correlated_hessian(k: int, tokens: int) -> np.ndarray:      # X = Z·A rounded to bf16, as test_gptq_gpu._factor builds it
    g = torch.Generator(device="cuda").manual_seed(k)
    a = torch.randn((k, k), generator=g, device="cuda", dtype=torch.float64) / np.sqrt(k)
    xd = (torch.randn((tokens, k), generator=g, device="cuda", dtype=torch.float64) @ a).to(torch.bfloat16).double()
    return (xd.T @ xd).cpu().numpy()


def _residual(u: np.ndarray, hd: np.ndarray) -> float:
    ul = u.astype(np.longdouble)
    return float(np.abs(ul @ hd.astype(np.longdouble) @ ul.T - np.eye(u.shape[0], dtype=np.longdouble)).max())


@pytest.mark.parametrize("k,tokens", [(100, 4096), (3 * NB + 7, 4096), (520, 4096), (300, 200)])
def test_residual_on_correlated_activations(k, tokens):
    torch.cuda.set_device(0)
    h = correlated_hessian(k, tokens)
    hd, u_host = gq.damped_hessian(h, 0.01), gq.factor(h, 0.01)
    u_dev, status = _factor_dev(hd)
    assert not isinstance(u_host, str) and status == 0 and bool((np.diag(u_dev) > 0).all()) and not np.tril(u_dev, -1).any()
    r_dev, r_host = _residual(u_dev, hd), _residual(u_host, hd)
    print(f"k {k} tokens {tokens}: residual device {r_dev:.3e} host {r_host:.3e} ratio {r_dev / r_host:.3f}")
    assert r_dev <= RESIDUAL_C * r_host, (r_dev, r_host)


@pytest.mark.parametrize("case", ["negative", "zero", "nan"])
def test_status_names_the_failing_pivot_and_the_next_call_is_clean(case):
    torch.cuda.set_device(0)
    k, j = 3 * NB + 7, NB + 5                                   # an index inside the second block
    if case == "negative":
        d = np.ones(k)
        d[j] = -1.0                                             # λ = 0.01·mean(diag) < 1: the damped pivot stays negative
        assert _factor_dev(np.diag(d))[1] == j + 1
        why = gq.factor_hip(torch.from_numpy(np.diag(d)).cuda())
        assert isinstance(why, str) and f"index {j}," in why, why
    elif case == "zero":
        assert _factor_dev(exact_case(k, j)[0])[1] == j + 1
    else:
        h = torch.from_numpy(exact_case(k)[0]).cuda()
        h[j, j + 2] = float("nan")
        assert gq.factor_hip(h) == "the calibration Hessian holds a non-finite value"
    u, status = _factor_dev(exact_case(k)[0])
    assert status == 0 and np.array_equal(u, exact_case(k)[1])


@pytest.mark.parametrize("kind", ["bfp4", "map"])
def test_device_factor_through_the_sweep(kind):
    torch.cuda.set_device(0)
    n, k = 64, 300
    w, x_cal, _x_eval = correlated_case(12, n=n, k=k)           # seed 12: margins 2.8e-5 (bfp4) and 2⁻¹⁹ (map), found on the CPU
    w, xd = w.to(torch.bfloat16), x_cal.double()
    h = (xd.T @ xd).numpy()
    codes = _codes(n, k, kind, n * k)
    u_host = gq.factor(h)
    u_dev = gq.factor_hip(torch.from_numpy(h).cuda())
    assert not isinstance(u_host, str) and not isinstance(u_dev, str), (u_host, u_dev)
    _q, _loss, margin = gq.sweep_emulation(w, u_host, codes)
    assert margin.min() > 2.0 ** -20, margin.min()              # every row's decisions are clear: nothing is masked below
    what_h, loss_h = gq.sweep_hip(w.cuda(), u_host, codes)
    what_d, loss_d = gq.sweep_hip(w.cuda(), u_dev, codes)
    assert np.array_equal(what_d.cpu().numpy().view(np.uint32), what_h.cpu().numpy().view(np.uint32))
    lh, ld = loss_h.cpu().numpy(), loss_d.cpu().numpy()
    assert np.all(np.abs(ld - lh) <= 1e-6 * lh), float(np.abs(ld / lh - 1).max())


def test_cli_gptq_factor_device_gives_the_host_rows(tmp_path):
    docs = {}
    for factor in ("host", "device"):
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), "synthetic:tiny", "synthetic:300",
                            "model.layers.1.attn.q", "--backend", "hip", "-c", "bfp8", "bfp4", "bfp2", "--gptq", "--gptq-factor", factor,
                            "--calib-io", "synthetic:300:1", "--out-dir", str(tmp_path / factor)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        docs[factor] = json.loads((tmp_path / factor / "layer_output_error.json").read_text())
    assert [docs[f]["gptq_factor"] for f in docs] == ["host", "device"] and len(docs["host"]["ops"]) == len(docs["device"]["ops"]) == 1
    for oh, od in zip(docs["host"]["ops"], docs["device"]["ops"]):
        names = [x["candidate"] for x in oh["rows"]]
        assert names == [x["candidate"] for x in od["rows"]] and [c for c in names if c.startswith("gptq:")] == ["gptq:bfp8", "gptq:bfp4", "gptq:bfp2"]
        for rh, rd in zip(oh["rows"], od["rows"]):
            assert (rh["bytes"], rh["pcc"], rh["mae"], rh["atol"]) == (rd["bytes"], rd["pcc"], rd["mae"], rd["atol"]), (rh, rd)
            if rh["candidate"].startswith("gptq:"):
                assert abs(rd["calib_loss"] - rh["calib_loss"]) <= 1e-6 * rh["calib_loss"]
