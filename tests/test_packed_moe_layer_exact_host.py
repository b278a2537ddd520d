"""CPU-only: the float64 reference of tests/moe_layer_cases.py holds its own conditions, and the emulation of every packed MLP and
MoE module equals it - to the bit on the exact tier, within the derived bound on the silu tier - in both `stored` orientations and
both types.  What the GPU file asks of the kernels, asked of the emulation first: a case that lost its point fails here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import packed
from tests import moe_layer_cases as mc
from tests.glu_chunked_cases import chunks

BF16 = torch.bfloat16


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return t if dtype is None else t.to(dtype)


def _f64(y) -> np.ndarray:
    return y.double().numpy() if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float64)


@pytest.mark.parametrize("layer,T,K", mc.PAIRS)
def test_the_conditions_of_the_exact_tier_hold(layer, T, K):
    count = mc.LAYERS[layer][0]
    ids = mc.exact_inputs(layer, T, K)[1]
    sizes = mc.check_routing(ids, count)
    group_rows = np.concatenate([[0], np.cumsum(sizes)])
    hot = int(np.diff(chunks(group_rows, T * K)).max())
    assert hot == {(3, 2): 1, (5, 3): 1, (32, 8): 6, (37, 2): 2, (130, 8): 23}[(T, K)]      # (32, 8): a second and a third chunk, and more
    assert (T * K <= mc.DECODE_MAX_ROWS) == ((T, K) != (130, 8)) and (T, K) != (32, 8) or T * K == mc.DECODE_MAX_ROWS
    room = mc.headroom(layer, T, K)
    print(f"headroom: {layer} (T, K) = ({T}, {K}): log2 of the largest quotients, projection / down / combine = " + " / ".join(f"{v:.1f}" for v in room))
    assert max(room) < 24


def test_the_two_orientations_multiply_by_one_matrix():
    """Both are packed from ONE W: each orientation's unpacked experts are the oracle's quantisation of W (of Wᵀ) under its own map,
    and where both maps keep bf16 the two hold W itself.  (bfp2 groups run along k in one and along n in the other: elsewhere the
    two Ŵ may differ, and each reference multiplies by its own.)"""
    for layer in mc.LAYERS:
        for tier in ("exact", "silu"):
            both = {s: mc.what(layer, tier, s) for s in mc.STORED}
            for p, w in enumerate(mc.weights(layer, tier)):
                rows = packed.unpack_batch(mc.experts(layer, tier, "rows")[p])
                kn = packed.unpack_batch_transposed(mc.experts(layer, tier, "transpose")[p])
                assert np.array_equal(rows.astype(np.float64), both["rows"][p]) and np.array_equal(kn.astype(np.float64), both["transpose"][p])
                m_rows, m_kn = mc.maps(layer, "rows")[p], mc.maps(layer, "transpose")[p]
                n, k = w.shape[1:]
                plain = (np.repeat(np.repeat(m_rows, 32, axis=1), 32, axis=2)[:, :n, :k] == 0) & \
                        (np.repeat(np.repeat(m_kn, 32, axis=1), 32, axis=2)[:, :k, :n].transpose(0, 2, 1) == 0)
                w16 = mc._bf16(w.astype(np.float64))
                assert plain.any() and np.array_equal(both["rows"][p][plain], w16[plain]) and np.array_equal(both["transpose"][p][plain], w16[plain])
                if tier == "exact":                       # on the grid only bfp2 moves a value
                    assert not np.array_equal(both["rows"][p], both["transpose"][p])


@pytest.mark.parametrize("layer,T,K", mc.PAIRS)
def test_the_emulated_layer_equals_the_exact_reference(layer, T, K):
    x, ids, w, base = mc.exact_inputs(layer, T, K)
    xt, wt = _t(x, BF16), _t(w)
    for stored in mc.STORED:
        ex = mc.experts(layer, "exact", stored)
        for expert_dtype in mc.DTYPES:
            for out_dtype in mc.DTYPES:
                moe = packed.PackedMoE(*ex, act="none", out_dtype=out_dtype, expert_dtype=expert_dtype, backend="emulation", stored=stored)
                for bi, kind in enumerate(mc.BASES):
                    want = mc.exact_want(layer, stored, T, K, expert_dtype, out_dtype, kind is not None)[0]
                    b = None if kind is None else _t(base, BF16 if kind == "bfloat16" else torch.float32)
                    y = moe(xt, _t(ids) if bi % 2 else _t(ids.astype(np.int32)), wt, base=b)
                    assert str(y.dtype) == "torch." + out_dtype and np.array_equal(_f64(y), want.astype(np.float64)), (stored, expert_dtype, out_dtype, kind)


@pytest.mark.parametrize("layer,T,K", mc.PAIRS)
def test_the_emulated_expert_modules_equal_the_exact_rows(layer, T, K):
    x, ids, _w, _base = mc.exact_inputs(layer, T, K)
    count = mc.LAYERS[layer][0]
    group_rows, R, token, expert = mc.rows_of_plan(ids, count)
    xs = _t(x[token], BF16)
    for stored in mc.STORED:
        d = mc.exact_rows(layer, stored, T, K)[0][token, expert]
        cls = packed.PackedExpertsMLP if stored == "rows" else packed.PackedExpertsMatmulMLP
        for out_dtype in mc.DTYPES:
            mlp = cls(*mc.experts(layer, "exact", stored), act="none", out_dtype=out_dtype, backend="emulation")
            y = mlp(xs, [int(v) for v in group_rows])
            assert tuple(y.shape) == (R, mc.LAYERS[layer][3]) and np.array_equal(_f64(y), mc._bf16(d) if out_dtype == "bfloat16" else d), (stored, out_dtype)


@pytest.mark.parametrize("layer", tuple(mc.LAYERS))
def test_the_emulated_dense_modules_equal_the_references(layer):
    for stored in mc.STORED:
        cls = packed.PackedMLP if stored == "rows" else packed.PackedMatmulMLP
        for tier, act in (("exact", "none"), ("silu", "silu")):
            one = mc.dense_experts(layer, tier, stored)
            for out_dtype in mc.DTYPES:
                for decode_kernel in ("pair", "fused"):
                    mlp = cls(*one, act=act, out_dtype=out_dtype, backend="emulation", decode_kernel=decode_kernel)
                    for m in mc.DENSE_M:
                        x, want, bound = mc.dense_want(layer, tier, stored, m, out_dtype, act)
                        err = np.abs(_f64(mlp(_t(x, BF16))) - want)
                        assert err.shape == (m, mc.LAYERS[layer][3]) and np.all(err <= (0.0 if bound is None else bound)), (stored, tier, out_dtype, decode_kernel, m)


@pytest.mark.parametrize("layer,T,name", mc.SILU_CASES)
def test_the_emulated_layer_is_within_the_silu_bound_and_an_exchange_is_not(layer, T, name):
    x, _logits, _bias, base, ids, w = mc.silu_inputs(layer, T, name)
    sizes = np.bincount(ids.reshape(-1), minlength=mc.LAYERS[layer][0])
    assert (T * ids.shape[1] <= mc.DECODE_MAX_ROWS) == (T != 130) and (T < 37 or sizes.max() > 32)
    for stored in mc.STORED:
        ex = mc.experts(layer, "silu", stored)
        for expert_dtype in mc.DTYPES:
            for out_dtype in mc.DTYPES:
                moe = packed.PackedMoE(*ex, act="silu", out_dtype=out_dtype, expert_dtype=expert_dtype, backend="emulation", stored=stored)
                for b in (None, base):
                    mc.check_exchange_is_seen(layer, stored, T, name, ids, w, b, expert_dtype, out_dtype)
                    want, bound = mc.silu_want(layer, stored, T, name, ids, w, b, expert_dtype, out_dtype)
                    y = moe(_t(x, BF16), _t(ids), _t(w), base=None if b is None else _t(b, BF16))
                    assert np.all(np.abs(_f64(y) - want) <= bound), (stored, expert_dtype, out_dtype, b is None)
                    exchanged = packed.PackedMoE(ex[1], ex[0], ex[2], act="silu", out_dtype=out_dtype, expert_dtype=expert_dtype, backend="emulation",
                                                 stored=stored)(_t(x, BF16), _t(ids), _t(w), base=None if b is None else _t(b, BF16))
                    assert (np.abs(_f64(exchanged) - want) > bound).any(axis=1).all(), "gate and up exchanged pass the bound"


@pytest.mark.parametrize("layer,T,name", mc.SILU_CASES)
def test_the_emulated_expert_modules_are_within_the_silu_bound(layer, T, name):
    x, _logits, _bias, _base, ids, _w = mc.silu_inputs(layer, T, name)
    group_rows, R, token, expert = mc.rows_of_plan(ids, mc.LAYERS[layer][0])
    xs = _t(x[token], BF16)
    for stored in mc.STORED:
        d, e_d = (a[token, expert] for a in mc.silu_rows(layer, stored, T, name))
        cls = packed.PackedExpertsMLP if stored == "rows" else packed.PackedExpertsMatmulMLP
        for out_dtype in mc.DTYPES:
            want, bound = mc._store_bf16(d, e_d) if out_dtype == "bfloat16" else (d, e_d)
            y = cls(*mc.experts(layer, "silu", stored), act="silu", out_dtype=out_dtype, backend="emulation")(xs, [int(v) for v in group_rows])
            assert tuple(y.shape) == (R, mc.LAYERS[layer][3]) and np.all(np.abs(_f64(y) - want) <= bound), (stored, out_dtype)
