"""GPTQ in the transposed BFP layout on the host: a diagonal Hessian gives the transposed round-to-nearest weights, Σ loss = Σ δ H_d δᵀ,
and evaluate_op's opt-in rows (gptq_transpose) replace the "row-layout only" entries."""
from __future__ import annotations

import numpy as np
import pytest

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd.compression_algorithms.config import CompressionConfig
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import evaluate_op, quantize_transposed
from tests.test_gptq_host import ALL, correlated_case, signed_zero_equal
from tests.test_output_error_transpose_host import FMTS, _ops


@pytest.mark.parametrize("kind", ["bfp8", "bfp4", "bfp2", "map"])
def test_diagonal_hessian_gives_transposed_rtn(kind):
    n, k = 70, 100
    rng = np.random.default_rng(k)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[16:32, 3] = 0.0                                              # an all-zero column group
    w[4, 5] = -0.0
    u = gq.factor(np.diag(rng.random(k) + 0.5))
    if kind == "map":
        codes = rng.integers(0, 4, size=bm.tiles_hw(k, n)).astype(np.int8)
        want = bm.reconstruct_emulation(w, codes, "transpose")
    else:
        codes = gq.constant_codes_transposed(n, k, kind)
        want = quantize_transposed(w, kind)
    q, loss, margin = gq.sweep_emulation_transposed(w, u, codes)
    assert signed_zero_equal(q, want)
    assert loss.shape == (n,) and np.all(np.isfinite(loss)) and margin.shape == (5,) and np.all(margin >= 0)


@pytest.mark.parametrize("seed", range(2))
def test_loss_identity_and_fixed_point(seed):
    w, x_cal, _ = correlated_case(seed, n=70, k=100, tokens=500)
    h, _m = gq.gram_full_emulation([Chunk(x=x_cal)], 100)
    u, hd = gq.factor(h), gq.damped_hessian(h)
    rng = np.random.default_rng(seed)
    for codes in [gq.constant_codes_transposed(70, 100, f) for f in ALL] + [rng.integers(0, 4, size=(4, 3)).astype(np.int8)]:
        q, loss, _margin = gq.sweep_emulation_transposed(w, u, codes)
        want = gq.quadratic_loss(w, q, hd)
        assert abs(loss.sum() - want.sum()) <= 1e-9 * want.sum()              # the row sweep's tolerance (test_gptq_host.py)
        assert signed_zero_equal(bm.reconstruct_emulation(q, codes, "transpose"), q)


def test_evaluate_op_opt_in_rows(tmp_path):
    _model, _io, index, ops, cal = _ops(tmp_path)
    cfg = CompressionConfig(algorithm="mixed-tile-greedy", params={"metric": "pcc", "threshold": 0.999, "layout": "transpose"},
                            quantization_formats=FMTS, seed=123, random_seed=False)
    op = ops[0]
    res = evaluate_op(index, op, ["bf16", "bfp8", "bfp4"], cfg, budgets=(9,), calib=cal[op.op], gptq=True, transpose=True, gptq_transpose=True)
    rows = {r.candidate: r for r in res.rows}
    assert [c for c in rows if c.startswith("gptq:")] == ["gptq:bfp8", "gptq:bfp4", "gptq:bfp8+transpose", "gptq:bfp4+transpose",
                                                          "gptq:map:mixed-tile-greedy+transpose", "gptq:budget:9:output", "gptq:budget:9:output+transpose"]
    assert res.budget_skipped == []
    for name, r in rows.items():
        if name.startswith("gptq:"):
            assert r.bytes == rows[name[len("gptq:"):]].bytes and r.extra["calib_loss"] >= 0.0 and 0.0 < r.pcc <= 1.0
            assert r.extra.get("layout") == ("transpose" if name.endswith("+transpose") else None)
