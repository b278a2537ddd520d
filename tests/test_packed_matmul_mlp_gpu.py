"""GPU: the modules over packed (k, n) weights — packed.PackedMatmulMLP, packed.PackedExpertsMatmulMLP and
packed.PackedMoE(stored="transpose") — against their written-out compositions, on the words.

  * PackedMatmulMLP, both decode_kernel values, above and inside the skinny range: glu_matmul(kernel="auto") (or glu_matmul_skinny)
    into bf16, then matmul(kernel="auto") with the (hidden, k_out) down matrix; leading dimensions kept; m = 0 empty;
  * PackedExpertsMatmulMLP on both sides of decode_max_rows: glu_matmul_grouped + matmul_grouped_wide, or glu_matmul_grouped_skinny +
    matmul_grouped(kernel="walk"); a pack_batch_transposed list goes in as it is; T = 0 empty;
  * PackedMoE(stored="transpose") equals plan → dispatch → PackedExpertsMatmulMLP → combine written out with the sort on the host:
    dropped ids, a token that names an expert twice, a base, T = 1 and T = 70; T = 130 with K = 8: S = 1040, the three-kernel plan and
    the combine's second batch of four slots inside a forward; stored="rows" still builds PackedExpertsMLP.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_packed_glu_gpu import _bits, _x_dev
from tests.test_packed_grouped_gpu import _rows_dev
from tests.test_packed_moe_gpu import _bf16_valued, _bf16_words, _want_combine, _want_plan

pytestmark = pytest.mark.gpu
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
ACTS = ("silu", "none")
COUNT, K_IN, HIDDEN, K_OUT = 5, 140, 72, 40


@functools.lru_cache(maxsize=None)
def _single():
    """(P̂g, P̂u (k, hidden), P̂d (hidden, k_out)) on the device."""
    wg, wu, wd = gen("heavy_f32", 11, (HIDDEN, K_IN)), gen("heavy_f32", 12, (HIDDEN, K_IN)), gen("heavy_f32", 13, (K_OUT, HIDDEN))
    return (packed.pack_transposed(wg, random_map((K_IN, HIDDEN), 14), backend="hip"),
            packed.pack_transposed(wu, random_map((K_IN, HIDDEN), 15), backend="hip"),
            packed.pack_transposed(wd, random_map((HIDDEN, K_OUT), 16), backend="hip"))


@functools.lru_cache(maxsize=None)
def _experts():
    """Three pack_batch_transposed lists: gate and up (k, hidden), down (hidden, k_out)."""
    wg = np.stack([gen("heavy_f32", 30 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wu = np.stack([gen("heavy_f32", 40 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wd = np.stack([gen("heavy_f32", 50 + i, (K_OUT, HIDDEN)) for i in range(COUNT)])
    maps = [np.stack([random_map(shape, seed + i) for i in range(COUNT)])
            for shape, seed in (((K_IN, HIDDEN), 33), ((K_IN, HIDDEN), 43), ((HIDDEN, K_OUT), 53))]
    assert not np.array_equal(maps[0][0], maps[0][1])
    return tuple(packed.pack_batch_transposed(torch.from_numpy(w).cuda(), m, backend="hip") for w, m in zip((wg, wu, wd), maps))


def test_packed_matmul_mlp_is_its_written_out_composition():
    gate, up, down = _single()
    m = 70
    x = _x_dev(to_bf16_valued(gen("normal_f32", 93, (m, K_IN)) * 40))
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            for decode_kernel in packed.MATMUL_MLP_DECODE_KERNELS:
                mlp = packed.PackedMatmulMLP(gate, up, down, act=act, out_dtype=out_dtype, decode_kernel=decode_kernel)
                assert mlp.backend == "hip" and (mlp.in_features, mlp.hidden_features, mlp.out_features) == (K_IN, HIDDEN, K_OUT)
                for rows in (m, 7, 32, 33):              # above, inside, at the end of and just past the skinny range
                    if decode_kernel == "fused" and rows <= packed.AUTO_GLU_MATMUL_SKINNY_MAX_M:
                        h = packed.glu_matmul_skinny(x[:rows], gate, up, act=act, out_dtype="bfloat16")
                    else:
                        h = packed.glu_matmul(x[:rows], gate, up, act=act, out_dtype="bfloat16", kernel="auto")
                    want = packed.matmul(h, down, out_dtype=out_dtype, kernel="auto")
                    y = mlp(x[:rows])
                    assert tuple(y.shape) == (rows, K_OUT) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), (act, out_dtype, rows)
                    # both decode kernels give the same words
                    pair = packed.glu_matmul(x[:rows], gate, up, act=act, out_dtype="bfloat16", kernel="auto")
                    assert np.array_equal(_bits(h), _bits(pair)), (act, rows, decode_kernel)
                assert np.array_equal(_bits(mlp(x.reshape(7, 10, K_IN)).reshape(m, K_OUT)), _bits(mlp(x)))
                empty = mlp(x[:0])
                assert tuple(empty.shape) == (0, K_OUT) and empty.dtype == dtype and empty.is_cuda


def test_packed_experts_matmul_mlp_on_both_sides_of_decode_max_rows():
    gates, ups, downs = _experts()                       # the pack_batch_transposed lists, as they are
    rows_wide, rows_decode = (0, 3, 3, 131, 132, 200), (0, 3, 3, 35, 36, 70)
    x = _x_dev(to_bf16_valued(gen("normal_f32", 97, (200, K_IN)) * 8))
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            experts = packed.PackedExpertsMatmulMLP(gates, ups, downs, act=act, out_dtype=out_dtype, decode_max_rows=70)
            assert experts.backend == "hip"
            assert (experts.count, experts.in_features, experts.hidden_features, experts.out_features) == (COUNT, K_IN, HIDDEN, K_OUT)
            h = packed.glu_matmul_grouped(x, list(rows_wide), gates, ups, act=act, out_dtype="bfloat16", kernel="fused")
            want = packed.matmul_grouped_wide(h, list(rows_wide), downs, out_dtype=out_dtype)
            for r in (list(rows_wide), _rows_dev(rows_wide)):
                y = experts(x, r)
                assert tuple(y.shape) == (200, K_OUT) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), (act, out_dtype, "wide")
            xs = x[:70]
            h = packed.glu_matmul_grouped_skinny(xs, list(rows_decode), gates, ups, act=act, out_dtype="bfloat16")
            want = packed.matmul_grouped(h, list(rows_decode), downs, out_dtype=out_dtype, kernel="walk")
            for r in (list(rows_decode), _rows_dev(rows_decode)):
                y = experts(xs, r)
                assert tuple(y.shape) == (70, K_OUT) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), (act, out_dtype, "decode")
            always_wide = packed.PackedExpertsMatmulMLP(gates, ups, downs, act=act, out_dtype=out_dtype)
            h = packed.glu_matmul_grouped(xs, list(rows_decode), gates, ups, act=act, out_dtype="bfloat16", kernel="fused")
            want = packed.matmul_grouped_wide(h, list(rows_decode), downs, out_dtype=out_dtype)
            assert np.array_equal(_bits(always_wide(xs, list(rows_decode))), _bits(want))
            empty = experts(x[:0], [0] * (COUNT + 1))
            assert tuple(empty.shape) == (0, K_OUT) and empty.dtype == dtype
    assert tuple(packed.glu_matmul_grouped(x[:0], [0] * (COUNT + 1), gates, ups).shape) == (0, HIDDEN)


def _layer_want(x, ids, w, base, expert_dtype, out_dtype, decode_max_rows):
    """Sort on the host, PackedExpertsMatmulMLP on the sorted rows with a host group_rows, the NumPy combine."""
    T, K = ids.shape
    group_rows, row_of, src = _want_plan(ids, COUNT)
    R = int(group_rows[-1])
    assert R > 0
    xg = x[torch.from_numpy(src[:R].astype(np.int64) // K).cuda()]
    mlp = packed.PackedExpertsMatmulMLP(*_experts(), out_dtype=expert_dtype, decode_max_rows=decode_max_rows)
    ys_r = mlp(xg, [int(v) for v in group_rows]).float().cpu().numpy()
    ys = np.zeros((T * K, K_OUT), dtype=np.float32)
    ys[:R] = ys_r
    with np.errstate(all="ignore"):
        acc = _want_combine(row_of, w, ys, base, T, K)
    return acc.view(np.int32) if out_dtype == "float32" else _bf16_words(acc).reshape(T, K_OUT)


def _layer_inputs(T, K, kind, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", seed, (T, K_IN)) * 50)).to(torch.bfloat16).cuda()
    if kind == "uniform":
        ids = rng.integers(0, COUNT, size=(T, K)).astype(np.int64)
        ids[0] = ids[0, 0]                               # a token that names one expert K times
    else:                                                 # experts 1 and 3 stay empty, some slots name experts of another rank
        ids = rng.choice(np.array([0, 2, 4, -1, COUNT, COUNT + 3], dtype=np.int64), size=(T, K))
        ids[0] = [2, -1]
        assert not np.isin(ids, (1, 3)).any() and (ids < 0).any()
    w = rng.random((T, K)).astype(np.float32) + 0.25
    base = _bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))
    return x, ids, w, base


@pytest.mark.parametrize("T,decode_max_rows,kind", ((70, None, "uniform"), (1, 64, "uniform"), (70, None, "sparse"), (1, 64, "sparse"), (70, 200, "sparse")))
def test_packed_moe_stored_transpose_is_sort_experts_combine(T, decode_max_rows, kind):
    K = 2
    x, ids, w, base = _layer_inputs(T, K, kind, 7 * T + K)
    ids_d, w_d = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()
    for expert_dtype in ("float32", "bfloat16"):
        for out_dtype in ("bfloat16", "float32"):
            moe = packed.PackedMoE(*_experts(), out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=decode_max_rows, stored="transpose")
            assert type(moe.experts).__name__ == "PackedExpertsMatmulMLP" and moe.stored == "transpose"
            assert moe.backend == "hip" and (moe.count, moe.in_features, moe.out_features) == (COUNT, K_IN, K_OUT)
            for with_base in (False, True):
                want = _layer_want(x, ids, w, base if with_base else None, expert_dtype, out_dtype, decode_max_rows)
                based = torch.from_numpy(base).cuda().to(torch.bfloat16) if with_base else None
                y = moe(x, ids_d, w_d, base=based)
                assert tuple(y.shape) == (T, K_OUT) and y.dtype == (torch.float32 if out_dtype == "float32" else torch.bfloat16)
                assert np.array_equal(_bits(y), want), (expert_dtype, out_dtype, with_base, np.argwhere(_bits(y) != want)[:4])
                assert np.array_equal(_bits(moe(x, ids_d.to(torch.int32), w_d, base=based)), want), "int32 ids give other words"
    empty = moe(x[:0], ids_d[:0], w_d[:0])
    assert tuple(empty.shape) == (0, K_OUT)


def test_packed_moe_stored_transpose_above_one_run():
    """T = 130, K = 8 (S = 1040): the three-kernel plan and the combine's second batch of slots inside a forward over (k, n) experts."""
    T, K = 130, 8
    assert T * K > hb.MOE_RUN and K > 4
    x, ids, w, base = _layer_inputs(T, K, "uniform", 7 * T + K)
    ids[1, ::3] = (-1, COUNT, COUNT + 3)                 # a token with dropped slots in either batch
    moe = packed.PackedMoE(*_experts(), out_dtype="bfloat16", expert_dtype="float32", stored="transpose", max_tokens=1)
    want = _layer_want(x, ids, w, base, "float32", "bfloat16", None)
    y = moe(x, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), base=torch.from_numpy(base).cuda().to(torch.bfloat16))
    assert tuple(y.shape) == (T, K_OUT) and np.array_equal(_bits(y), want), np.argwhere(_bits(y) != want)[:4]


def test_stored_rows_is_still_the_row_layout_layer_and_a_wrong_word_is_refused():
    from tests.test_packed_moe_gpu import _experts as row_experts

    moe = packed.PackedMoE(*row_experts())
    assert type(moe.experts).__name__ == "PackedExpertsMLP" and moe.stored == "rows"
    assert type(packed.PackedMoE(*row_experts(), stored="rows").experts).__name__ == "PackedExpertsMLP"
    with pytest.raises(hb.MtqError, match="stored must be one of"):
        packed.PackedMoE(*_experts(), stored="columns")
    with pytest.raises(hb.MtqError, match="down batch must hold"):
        packed.PackedMoE(*_experts())                    # (k, n) experts under the default word: the shapes do not fit the row layout
