"""AWQ for BFP on the MI355X: mtq_awq_quantize bit for bit against the host oracle, mtq_awq_losses exactly on grid inputs and within a
derived rounding bound on heavy-tailed weights, and the routes (evaluate_op, packing, PackedLinear).

Exact losses: X integers with |x| ≤ 4 and W on the 2⁻⁸ grid with |w| < 1 keep every image on the grid, so every output, every r − q and
(below 2⁵³ grid units, asserted per case) every sum is exact: hip must equal the oracle bit for bit.
Rounding bound: with ε = ε_r + ε_q the per-output bound of the fused kernel's float32 accumulation ((k + 2)·2⁻²⁴·(1 + 2⁻⁷)·
max Σ|x·w|) and d the oracle's r − q, |(d + δ)² − d²| ≤ 2ε|d| + ε² per output and the float64 sums add 64·MN·2⁻⁵³·loss."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import awq, hip_backend as hb, packed
from quantization_analysis_amd.budget_maps import gram_blocks_emulation
from quantization_analysis_amd.gptq import constant_codes
from quantization_analysis_amd.layer_io import Chunk, OpIO
from quantization_analysis_amd.output_error import evaluate_op

pytestmark = pytest.mark.gpu
FORMS = ("bfp8", "bfp4", "bfp2", "map")


class _Index:
    """The two calls evaluate_op makes on a model index, over one in-memory weight."""

    def __init__(self, w):
        self.w = w

    def shape_dtype(self, name):
        return tuple(self.w.shape), self.w.dtype

    def load(self, name, device=None):
        return self.w if device is None else self.w.to(device)


def _codes(rng, n, k, form):
    return rng.integers(0, 4, (-(-n // 32), -(-k // 32))).astype(np.int8) if form == "map" else constant_codes(n, k, form)


def _grid_case(rng, m, n, k, g):
    x = torch.from_numpy(rng.integers(-4, 5, (m, k)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy(rng.integers(-255, 256, (n, k)).astype(np.float32) / 256.0)
    p = rng.integers(0, 8, (g, k)).astype(np.int8)
    p[0] = 0
    return x, w, p


@pytest.mark.parametrize("kind", ["bf16", "float32", "heavy"])
@pytest.mark.parametrize("n, k", [(1, 16), (33, 40), (70, 200)])
def test_quantize_matches_the_oracle_bit_for_bit(n, k, kind):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + k)
    w = rng.standard_t(2, (n, k)) * 0.02 if kind == "heavy" else rng.standard_normal((n, k))
    # groups on both sides of the exact-scaling route's borders (E = 48 and 200), all-zero groups and lone zeros
    w = np.ldexp(w, np.repeat(rng.choice([-90, -82, -78, 0, 0, 66, 71, 76], (n, -(-k // 16))), 16, axis=1)[:, :k]).astype(np.float32)
    w[rng.random((n, k)) < 0.05] = 0.0
    w[0, :16] = 0.0
    wt = torch.from_numpy(w).to(torch.bfloat16 if kind == "bf16" else torch.float32)
    held = torch.zeros((n, k + 24), dtype=wt.dtype, device="cuda")      # a padded ld
    held[:, :k] = wt
    for form in FORMS:
        codes, p = _codes(rng, n, k, form), rng.integers(0, 8, k).astype(np.int8)
        got = awq.quantize_hip(held[:, :k], codes, p).cpu().numpy()
        want = awq.quantize_emulation(wt, codes, p)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), form


@pytest.mark.parametrize("k", [16, 33, 65, 200])
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("m", [1, 129, 300])
def test_losses_are_exact_on_the_grid(m, n, k):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(m * 7 + n * 3 + k)
    S = hb.awq_slots()      # G′ = S + 1 crosses a launch border, for both storage types
    for g, dtype, form in ((1, torch.bfloat16, "bfp8"), (S, torch.float32, "map"), (S + 1, torch.bfloat16, "bfp2"), (S + 1, torch.float32, "bfp4")):
        x, w, p = _grid_case(rng, m, n, k, g)
        codes = _codes(rng, n, k, form)
        want, _ = awq.losses_emulation([Chunk(x=x)], w, codes, p)
        assert want.max() * 2.0 ** 16 < 2.0 ** 53
        got, tokens = awq.losses_hip([Chunk(x=x)], w.to(dtype), codes, p)
        assert tokens == m and np.array_equal(got.cpu().numpy(), want), (g, form, got.cpu().numpy(), want)


def test_losses_accumulate_over_chunks():
    torch.cuda.set_device(0)
    rng = np.random.default_rng(5)
    x, w, p = _grid_case(rng, 300, 70, 72, hb.awq_slots() + 1)
    codes = constant_codes(70, 72, "bfp4")
    want, _ = awq.losses_emulation([Chunk(x=x)], w, codes, p)
    one, _ = awq.losses_hip([Chunk(x=x)], w, codes, p)
    two, tokens = awq.losses_hip([Chunk(x=x[:129]), Chunk(x=x[:0]), Chunk(x=x[129:])], w, codes, p)
    assert tokens == 300 and torch.equal(one, two) and np.array_equal(one.cpu().numpy(), want)
    loss = torch.full((p.shape[0],), 3.0, dtype=torch.float64, device="cuda")   # ADDS into a non-zero vector
    hb.awq_losses(x.cuda(), w.cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(p).cuda(), loss)
    assert np.array_equal(loss.cpu().numpy(), want + 3.0)


def _bound(x, w, what, want_loss):
    x64, w64 = x.double().numpy(), w.double().numpy()
    eps = _eps_k(x64, w64) + _eps_k(x64, what)
    d = x64 @ (w64 - what).T
    return 2 * eps * np.abs(d).sum() + d.size * eps * eps + 64 * d.size * 2.0 ** -53 * want_loss


def _eps_k(xa, wa):
    return (xa.shape[1] + 2) * 2.0 ** -24 * (1 + 2.0 ** -7) * float((np.abs(xa) @ np.abs(wa).T).max())


@pytest.mark.parametrize("form", ["bfp8", "bfp2"])
def test_losses_within_the_rounding_bound_on_heavy_tailed_float32(form):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(9)
    m, n, k = 200, 100, 328
    x = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy((rng.standard_t(2, (n, k)) * 0.02).astype(np.float32))
    p = rng.integers(0, 8, (hb.awq_slots() + 2, k)).astype(np.int8)
    codes = constant_codes(n, k, form)
    want, _ = awq.losses_emulation([Chunk(x=x)], w, codes, p)
    got = awq.losses_hip([Chunk(x=x)], w, codes, p)[0].cpu().numpy()
    for g in range(p.shape[0]):
        bound = _bound(x, w, awq.quantize_emulation(w, codes, p[g]).astype(np.float64), want[g])
        print(form, g, got[g], want[g], abs(got[g] - want[g]), bound)
        assert abs(got[g] - want[g]) <= bound


def test_evaluate_op_awq_rows_on_hip_match_the_emulation(tmp_path):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(28)     # picked on the CPU: the oracle's best-to-second gap is clear of the bound for both formats
    n, k, m = 64, 128, 96
    w = torch.from_numpy((rng.standard_t(3, (n, k)) * 0.05).astype(np.float32))
    ops, xs = {}, {}
    for idx, split in enumerate(("calibration", "test")):
        x = rng.standard_normal((2 * k if idx == 0 else m, k)).astype(np.float32)
        x[:, [5, 77]] *= 48.0
        xs[split] = torch.from_numpy(x).to(torch.bfloat16)
        torch.save({"args": (xs[split],), "kwargs": {}, "output": (xs[split].float() @ w.T).to(torch.bfloat16)}, tmp_path / f"s{idx}.pt")
        ops[split] = OpIO(op="op", weight="op.weight", bias=None, samples=[(split, idx, tmp_path / f"s{idx}.pt")])
    index, fmts = _Index(w), ["bfp8", "bfp4"]
    rh = evaluate_op(index, ops["test"], fmts, None, "hip", calib=ops["calibration"], awq=True)
    re_ = evaluate_op(index, ops["test"], fmts, None, "emulation", calib=ops["calibration"], awq=True)
    assert [r.candidate for r in rh.rows] == [r.candidate for r in re_.rows] == fmts + ["recorded", "awq:bfp8", "awq:bfp4"]
    assert rh.budget_skipped == re_.budget_skipped == []
    xt, xc = xs["test"].float().numpy(), xs["calibration"]
    t = awq.channel_log2(*gram_blocks_emulation([Chunk(x=xc)], k))
    _alphas, table = awq.exponent_table(t[:k])
    for a, b, f in zip(rh.rows[-2:], re_.rows[-2:], fmts):
        codes = constant_codes(n, k, f)
        losses, _ = awq.losses_emulation([Chunk(x=xc)], w, codes, table)
        first, second = np.argsort(losses, kind="stable")[:2]
        room = sum(_bound(xc, w, awq.quantize_emulation(w, codes, table[g]).astype(np.float64), losses[g]) for g in (first, second))
        print(a.candidate, a.extra["g"], b.extra["g"], a.extra["calib_loss"], b.extra["calib_loss"], losses[second] - losses[first], room)
        assert b.extra["g"] == first and a.extra["calib_loss"] <= a.extra["rtn_calib_loss"] and a.bytes == rh.rows[fmts.index(f)].bytes
        assert a.extra["calib_tokens"] == b.extra["calib_tokens"] == 2 * k
        assert first > 0 and losses[second] - losses[first] > room       # the planted case: g* is decided, so hip must find it too
        assert a.extra["g"] == first and a.extra["shifted_channels"] == b.extra["shifted_channels"] > 0
        # the rows: LOE's bounds (test_output_error_gpu.py): mae / atol within ε_r + ε_q, pcc within 2ε_r/σ_r + 2ε_q/σ_q
        eps = _eps_k(xt, w.numpy()) + _eps_k(xt, awq.quantize_emulation(w, codes, table[first]))
        count, (sa, sb) = float(m * n), (np.asarray(a.sums), np.asarray(b.sums))
        ga, gb = hb.columns_from_sums(sa, count), hb.columns_from_sums(sb, count)
        sr, sq = np.sqrt(sb[1] / count - (sb[0] / count) ** 2), np.sqrt(sb[3] / count - (sb[2] / count) ** 2)
        f64 = 64 * count * 2.0 ** -53
        assert abs(ga["mae"] - gb["mae"]) <= eps + f64 * gb["mae"] and abs(ga["atol"] - gb["atol"]) <= eps + 2.0 ** -52 * gb["atol"]
        assert abs(ga["pcc"] - gb["pcc"]) <= 2 * eps / min(sr, sq) + f64 * np.sqrt(sb[1] * sb[3]) / count / (sr * sq)
    plain, off = evaluate_op(index, ops["test"], fmts, None, "hip"), evaluate_op(index, ops["test"], fmts, None, "hip", awq=False)
    assert [(r.candidate, r.sums) for r in off.rows] == [(r.candidate, r.sums) for r in plain.rows]


@pytest.mark.parametrize("form", ["bfp8", "map"])
def test_deployed_weight_and_packed_linear(form):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(2)
    m, n, k = 40, 64, 96
    x, w, p = _grid_case(rng, m, n, k, 2)
    codes, p_row = _codes(rng, n, k, form), p[1]
    what = awq.quantize_hip(w, codes, p_row)
    pt = packed.pack(awq.scale_weight(w.cuda(), p_row), codes, backend="hip")
    assert torch.equal(packed.unpack(pt, backend="hip").float(), torch.ldexp(what, torch.from_numpy(p_row.astype(np.int32)).cuda()))
    y = packed.PackedLinear(pt, in_exponents=p_row)(x.cuda())
    assert torch.equal(y.double().cpu(), x.double() @ what.double().cpu().T)
    assert "in_exponents" in repr(packed.PackedLinear(pt, in_exponents=p_row))
    with pytest.raises(ValueError):
        packed.PackedLinear(pt, in_exponents=np.full(k, 8))
    with pytest.raises(hb.MtqError):                                     # the kernels' precondition on W is checked, not assumed
        awq.quantize_hip(torch.full((n, k), float("inf")), codes, p_row)
