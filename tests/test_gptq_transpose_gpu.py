"""GPTQ in the transposed BFP layout on the MI355X: mtq_gptq_sweep_transposed against the host emulation on the same host-factorised U
(bitwise on the 16-row groups whose decisions are clear), the diagonal-H case against the transposed round-to-nearest kernels (which
pins the cross-lane exponent reduction, tails included), and evaluate_op's opt-in rows against the emulation backend."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb
from tests.test_budget_maps_host import loe_sse
from tests.test_gptq_gpu import _codes, _factor
from tests.test_gptq_host import signed_zero_equal
from tests.test_output_error_host import make_fixture

pytestmark = pytest.mark.gpu


CASES = [(70, 100, "f32", "bfp4"), (70, 100, "bf16", "map"), (300, 200, "bf16", "bfp2"), (300, 200, "f32", "map"),
         (300, 200, "f32", "bfp8"), (48, 1024, "bf16", "map"), (48, 1024, "f32", "bfp4")]


@pytest.mark.parametrize("n,k,wdt,kind", CASES)
def test_sweep_matches_emulation_on_clear_groups(n, k, wdt, kind):
    """The two routes differ only in float64 summation order (about k · 2⁻⁵³ relative, on values of at most 2⁸ steps), so a group whose
    margin exceeds 2⁻³⁰ steps must agree bit for bit; at most one group per case may be unclear (a condition, not a measurement: on a
    host float64 emulation with a host-generated U every group of the seven cases was clear at 2⁻³⁰; so it is with this test's
    device-generated U on the MI355X: 5 / 5 / 19 / 19 / 19 / 3 / 3 groups clear, least margin 9.5e-7 steps)."""
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + k)
    w = (rng.standard_normal((n, k + 3)) * 0.05).astype(np.float32)
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32).cuda()[:, 1: 1 + k]   # ldw > k, unaligned base
    codes = _codes(k, n, kind, n * k)                              # over Wᵀ's grid
    u = _factor(k)
    what, loss = gq.sweep_hip_transposed(wt, u, codes)
    what2, loss2 = gq.sweep_hip_transposed(wt.contiguous(), u, codes)
    got = what.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), what2.cpu().numpy().view(np.uint32)) and torch.equal(loss, loss2)
    want, want_loss, margin = gq.sweep_emulation_transposed(wt.cpu(), u, codes)
    clear = np.repeat(margin > 2.0 ** -30, 16)[:n]
    print(f"clear groups: {int((margin > 2.0 ** -30).sum())} of {margin.size}; least margin {margin.min():.3e}")
    assert (margin <= 2.0 ** -30).sum() <= 1, margin
    assert np.array_equal(got[clear].view(np.uint32), want[clear].view(np.uint32)), np.nonzero((got != want).any(axis=1) & clear)
    lh = loss.cpu().numpy()
    assert np.all(np.abs(lh[clear] - want_loss[clear]) <= 1e-9 * want_loss[clear] + 1e-300)
    # every row: bf16-exact, and a fixed point of the transposed quantiser
    assert torch.equal(what.to(torch.bfloat16).float(), what)
    again = hb.apply_assignment_transposed(what, codes) if kind == "map" else hb.quantize_transposed(what, kind)
    assert signed_zero_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("kind", ["bfp8", "bfp4", "bfp2", "map"])
@pytest.mark.parametrize("n,k,wdt", [(70, 100, "f32"), (300, 200, "bf16")])
def test_diagonal_hessian_gives_transposed_round_to_nearest(n, k, wdt, kind):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(k)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[16:32, 3] = 0.0                                              # a zeroed 16-row column group
    w[4, 5] = -0.0
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32).cuda()
    u = gq.factor(np.diag(rng.random(k) + 0.5))
    codes = _codes(k, n, kind, 7)
    what, _loss = gq.sweep_hip_transposed(wt, u, codes)
    want = hb.apply_assignment_transposed(wt, codes) if kind == "map" else hb.quantize_transposed(wt, kind)
    assert signed_zero_equal(what.cpu().numpy(), want.cpu().numpy())


def test_evaluate_op_gptq_transpose_rows_on_hip(tmp_path):
    torch.cuda.set_device(0)
    from quantization_analysis_amd.layer_io import select_ops
    from quantization_analysis_amd.model_source import build_model_index
    from quantization_analysis_amd.output_error import evaluate_op

    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp", "test")
    cal, _ = select_ops(index, io, "model.layers.0.mlp", "calibration")
    cal = {o.op: o for o in cal}
    fm = ["bf16", "bfp8", "bfp4", "bfp2"]
    for op in ops:
        kw = dict(budgets=(4.0,), calib=cal[op.op], gptq=True, transpose=True, gptq_transpose=True)
        rh = evaluate_op(index, op, fm, None, "hip", **kw)
        re_ = evaluate_op(index, op, fm, None, "emulation", **kw)
        names = [r.candidate for r in rh.rows]
        assert names[-8:] == ["gptq:bfp8", "gptq:bfp4", "gptq:bfp2", "gptq:bfp8+transpose", "gptq:bfp4+transpose", "gptq:bfp2+transpose",
                              "gptq:budget:4:output", "gptq:budget:4:output+transpose"], names
        assert [r.candidate for r in re_.rows] == names and rh.budget_skipped == []
        for a, b in zip(rh.rows[-8:], re_.rows[-8:]):
            assert a.bytes == b.bytes and a.extra.get("layout") == b.extra.get("layout")
            assert abs(a.extra["calib_loss"] - b.extra["calib_loss"]) <= 0.05 * b.extra["calib_loss"] + 1e-12, (a.candidate, a.extra, b.extra)
            assert abs(loe_sse(a.sums) - loe_sse(b.sums)) <= 0.05 * loe_sse(b.sums) + 1e-12, (a.candidate, a.sums, b.sums)
