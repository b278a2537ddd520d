"""GPU: the MoE routing kernels of csrc/mtq_moe.hip (mtq_moe_plan, mtq_moe_dispatch, mtq_moe_combine) and packed.PackedMoE on them.

The want-side is never the code under test: the plan is np.argsort(kind="stable") written out here, the dispatch a NumPy gather, the
combine a float32 NumPy loop in the contract's order, and the layer is the existing PackedExpertsMLP on a routing sorted on the host
followed by that loop.  Everything is compared as integer words.

  plan      (T, K, count) = (1, 1, 1), (1, 8, 256), (7, 2, 5), (64, 8, 256), (128, 8, 256): S = 1024, the last one-launch size,
            (129, 8, 256): the first three-kernel size, (300, 6, 300): more experts than a 256-thread block and no power of two,
            (4099, 8, 256): 33 runs, the last ragged; each with uniform ids, every slot on one expert, tokens that name one expert
            twice, and about a quarter of the ids replaced by -1, count and the id type's minimum and maximum; int32 and int64 ids;
            ids contiguous and as a view of a wider buffer; over a workspace of 0xFF bytes with sentinels behind it; twice, same words.
  dispatch  k = 8, 64, 300, 1000; x contiguous, a view of a wider buffer, and starting at an unaligned element; xs a pitched view
            of sentinels with sentinel rows behind it, x with rows behind it that must not be read; a hand-made src with -1, S and the
            int32 extremes.
  combine   n = 8, 72, 200, 1000; ys bf16 / float32, y float32 / bf16, base none / bf16 / float32; weights with negative values and
            exact zeros; rows of ys from R on hold NaN and Inf words; a row_of with -1, S and the int32 extremes; y a pitched view of
            sentinels, at an aligned and at an odd pitch (the 16-byte and the element path).
  layer     5 experts, 128 → 96 → 64, a different random map per expert: T = 37, K = 2 on the wide route, T = 3, K = 2 with
            decode_max_rows = 64 on the skinny route, a routing that leaves two experts empty and drops slots, both expert_dtypes, with
            a base, and leading dimensions (2, 5).
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

pytestmark = pytest.mark.gpu
ROUTINGS = ((1, 1, 1), (1, 8, 256), (7, 2, 5), (64, 8, 256), (128, 8, 256), (129, 8, 256), (300, 6, 300), (4099, 8, 256))
KINDS = ("uniform", "one", "twice", "dropped")
ID_TYPES = ((np.int32, torch.int32), (np.int64, torch.int64))
SENTINEL = 0xA5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _bits(t) -> np.ndarray:
    """The words of a device tensor: int16 for bf16, int32 for float32 and int32."""
    t = t.detach()
    return (t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)).cpu().numpy()


def _bf16_words(a32: np.ndarray) -> np.ndarray:
    """float32 (finite) → the bf16 words of its round-to-nearest-even, as int16."""
    u = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def _bf16_valued(a32: np.ndarray) -> np.ndarray:
    return (_bf16_words(a32).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _routing(T, K, count, kind, np_type, seed=0) -> np.ndarray:
    rng = np.random.default_rng(1000 * T + 10 * K + count + seed)
    ids = rng.integers(0, count, size=(T, K)).astype(np_type)
    if kind == "one":
        ids[:] = count - 1
    elif kind == "twice" and K > 1:
        ids[:, 1] = ids[:, 0]
    elif kind == "dropped":
        info = np.iinfo(np_type)
        bad = np.array([-1, count, info.min, info.max, count + 7, -count], dtype=np_type)
        drop = rng.random((T, K)) < 0.25
        drop.reshape(-1)[0] = True
        ids[drop] = bad[rng.integers(0, bad.size, size=int(drop.sum()))]
    return ids


def _want_plan(ids: np.ndarray, count: int):
    """(group_rows, row_of, src) by the contract's independent statement: the stable argsort of where(live, id, count)."""
    flat = ids.astype(np.int64).reshape(-1)
    S = flat.size
    live = (flat >= 0) & (flat < count)
    order = np.argsort(np.where(live, flat, count), kind="stable")
    R = int(live.sum())
    src = np.full(S, -1, dtype=np.int32)
    src[:R] = order[:R]
    row_of = np.full(S, -1, dtype=np.int32)
    row_of[order[:R]] = np.arange(R, dtype=np.int32)
    group_rows = np.zeros(count + 1, dtype=np.int32)
    group_rows[1:] = np.cumsum(np.bincount(flat[live], minlength=count))
    return group_rows, row_of, src


@pytest.mark.parametrize("T,K,count", ROUTINGS)
def test_plan_is_the_stable_sort_of_the_slots(T, K, count):
    S = T * K
    need = hb.moe_plan_workspace_bytes(T, K, count)
    assert need == ((S + 1023) // 1024 * count * 4 + 15) // 16 * 16 > 0
    buf = torch.empty((need + 64,), dtype=torch.uint8, device="cuda")
    for kind in KINDS:
        for np_type, torch_type in ID_TYPES:
            ids = _routing(T, K, count, kind, np_type)
            want = _want_plan(ids, count)
            if kind == "one":
                assert want[0][-1] == S and np.array_equal(want[2], np.arange(S))
            if kind == "dropped":
                assert want[0][-1] < S
            wide = torch.full((T, K + 3), count - 1, dtype=torch_type, device="cuda")      # live ids around the view: a misread shows
            wide[:, 1: 1 + K] = torch.from_numpy(ids).cuda()
            for view in (torch.from_numpy(ids).cuda(), wide[:, 1: 1 + K]):
                got = []
                for _ in range(2):
                    buf[:need] = 0xFF
                    buf[need:] = SENTINEL
                    plan = packed.moe_plan(view, count, workspace=buf[:need])
                    assert plan.on_device and (plan.tokens, plan.topk, plan.count, plan.slots) == (T, K, count, S)
                    got.append([t.cpu().numpy() for t in (plan.group_rows, plan.row_of, plan.src)])
                    assert bool((buf[need:] == SENTINEL).all()), "bytes behind the workspace were written"
                for g, w, name in zip(got[0], want, ("group_rows", "row_of", "src")):
                    assert g.dtype == np.int32 and g.shape == w.shape, name
                    assert np.array_equal(g, w), (kind, np_type.__name__, name, np.flatnonzero(g != w)[:8])
                assert all(np.array_equal(a, b) for a, b in zip(*got)), "two calls differ"


# ----------------------------------------------------------------------------- dispatch

DT, DK = 37, 3                                            # 111 rows: more than one workgroup at every k below


@functools.lru_cache(maxsize=None)
def _dispatch_case(k):
    S = DT * DK
    rng = np.random.default_rng(k)
    x = rng.integers(0, 1 << 16, size=(DT, k), dtype=np.uint16).astype(np.uint16)        # any words: a bit copy, NaN words included
    src = rng.integers(0, S, size=S).astype(np.int64)
    src[[0, 5, 17, 40, S - 1]] = [-1, S, I32_MIN, I32_MAX, S + 5]
    src[1], src[2] = S - 1, 0
    keep = (src >= 0) & (src < S)
    want = np.zeros((S, k), dtype=np.uint16)
    want[keep] = x[src[keep] // DK]
    return x, src.astype(np.int32), want


@pytest.mark.parametrize("k", (8, 64, 300, 1000))
def test_dispatch_copies_the_named_rows_and_zeroes_the_rest(k):
    S = DT * DK
    x, src, want = _dispatch_case(k)
    never = np.uint16(0x7FC1)                             # the words behind x: no output may hold them (x holds them nowhere either)
    x = np.where(x == never, np.uint16(1), x)
    want = np.where(want == never, np.uint16(1), want)
    src_d = torch.from_numpy(src).cuda()
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), src_d, src_d, DT, DK, 1)

    def as_dev(words):
        return torch.from_numpy(words.view(np.int16)).cuda().view(torch.bfloat16)

    behind = np.full((DT + 2, k + 8), never, dtype=np.uint16)
    behind[:DT, :k] = x
    odd = np.full((DT + 2, k + 5), never, dtype=np.uint16)
    odd[:DT, :k] = x
    flat = np.full((3 + (DT + 2) * k,), never, dtype=np.uint16)
    flat[3: 3 + DT * k] = x.reshape(-1)
    views = {"contiguous": as_dev(x), "wider": as_dev(behind)[:DT, :k], "odd pitch": as_dev(odd)[:DT, :k],
             "unaligned": as_dev(flat)[3: 3 + DT * k].view(DT, k)}
    for name, xd in views.items():
        y = packed.moe_dispatch(xd, plan)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (S, k)
        assert np.array_equal(_bits(y).view(np.uint16), want), (name, k)
        for pad in (8, 3):                                # a pitched xs of sentinels with sentinel rows behind it
            out = torch.full((S + 2, k + pad), -1.0, dtype=torch.bfloat16, device="cuda")
            fill = _bits(out)[0, 0]
            y = packed.moe_dispatch(xd, plan, out=out[:S, :k])
            got = _bits(out)
            assert np.array_equal(got[:S, :k].view(np.uint16), want), (name, k, pad)
            assert (got[S:] == fill).all() and (got[:, k:] == fill).all(), (name, k, pad, "xs was written outside S x k")


# ----------------------------------------------------------------------------- combine

CT, CK = 19, 4


@functools.lru_cache(maxsize=None)
def _combine_case(n):
    """Routing with drops, hand-made bad rows, weights, ys (float32 values that are bf16 values, so both storages hold them), bases."""
    S = CT * CK
    rng = np.random.default_rng(n)
    ids = _routing(CT, CK, 6, "dropped", np.int64, seed=n)
    _g, row_of, _s = _want_plan(ids, 6)
    R = int((row_of >= 0).sum())
    assert 0 < R < S
    row_of = row_of.copy()
    live = np.flatnonzero(row_of >= 0)
    row_of[live[[1, 4, 9]]] = [S, I32_MIN, I32_MAX]        # hand-made: skipped like the dropped slots
    w = rng.standard_normal((CT, CK)).astype(np.float32)
    w[rng.random((CT, CK)) < 0.2] = 0.0
    w[0, 0], w[1, 1] = -1.5, 0.0
    assert (w < 0).any() and (w == 0).any()
    ys = _bf16_valued(rng.standard_normal((S, n)).astype(np.float32) * 3)
    base = _bf16_valued(rng.standard_normal((CT, n)).astype(np.float32))
    poison = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0xFFC00000], dtype=np.uint32).view(np.float32)
    ys_dev = ys.copy()
    ys_dev[R:] = poison[rng.integers(0, 4, size=(S - R, n))]                  # never read: no kept slot names a row from R on
    return row_of, w, ys, ys_dev, base


def _want_combine(row_of, w, ys, base, T, K):
    """The contract's loop in NumPy's float32: product and sum rounded separately, j ascending, rows outside [0, S) skipped."""
    S = T * K
    acc = np.zeros((T, ys.shape[1]), dtype=np.float32) if base is None else base.astype(np.float32).copy()
    for t in range(T):
        for j in range(K):
            r = int(row_of[t * K + j])
            if 0 <= r < S:
                acc[t] = acc[t] + np.float32(w[t, j]) * ys[r]
    assert acc.dtype == np.float32 and np.isfinite(acc).all()
    return acc


@pytest.mark.parametrize("n", (8, 72, 200, 1000))
def test_combine_sums_in_slot_order_and_skips_what_is_no_row(n):
    S = CT * CK
    row_of, w, ys, ys_dev, base = _combine_case(n)
    row_d, w_d = torch.from_numpy(row_of).cuda(), torch.from_numpy(w).cuda()
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), row_d, row_d, CT, CK, 1)
    wants = {None: _want_combine(row_of, w, ys, None, CT, CK), "base": _want_combine(row_of, w, ys, base, CT, CK)}
    assert not np.array_equal(wants[None], wants["base"])
    for ys_type in (torch.bfloat16, torch.float32):
        ysd = torch.from_numpy(ys_dev).cuda().to(ys_type)                    # exact: bf16 values (NaN and Inf words stay NaN and Inf)
        for base_type in (None, torch.bfloat16, torch.float32):
            based = None if base_type is None else torch.from_numpy(base).cuda().to(base_type)
            want32 = wants[None if base_type is None else "base"]
            for out_dtype, torch_out in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
                want = want32.view(np.int32) if out_dtype == "float32" else _bf16_words(want32).reshape(CT, n)
                what = (n, ys_type, base_type, out_dtype)
                y = packed.moe_combine(ysd, w_d, plan, base=based, out_dtype=out_dtype)
                assert y.dtype == torch_out and tuple(y.shape) == (CT, n)
                assert np.array_equal(_bits(y), want), (what, np.argwhere(_bits(y) != want)[:4])
                for pad in (8, 3):                        # pitched y of sentinels: the 16-byte path and the element path
                    out = torch.full((CT + 2, n + pad), -3.0, dtype=torch_out, device="cuda")
                    fill = _bits(out)[0, 0]
                    packed.moe_combine(ysd, w_d, plan, base=based, out_dtype=out_dtype, out=out[:CT, :n])
                    got = _bits(out)
                    assert np.array_equal(got[:CT, :n], want), (what, pad)
                    assert (got[CT:] == fill).all() and (got[:, n:] == fill).all(), (what, pad, "y was written outside tokens x n")
        # operands at odd pitches and an unaligned start: the element path, the same words
        wide = torch.zeros((S, n + 3), dtype=ys_type, device="cuda")
        wide[:, :n] = ysd
        wpitch = torch.zeros((CT, CK + 1), dtype=torch.float32, device="cuda")
        wpitch[:, :CK] = w_d
        y = packed.moe_combine(wide[:, :n], wpitch[:, :CK], plan, out_dtype="float32")
        assert np.array_equal(_bits(y), wants[None].view(np.int32)), (n, ys_type, "odd pitches")


# ----------------------------------------------------------------------------- the layer

COUNT, K_IN, HIDDEN, K_OUT = 5, 128, 96, 64


@functools.lru_cache(maxsize=None)
def _experts():
    wg = np.stack([gen("heavy_f32", 30 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wu = np.stack([gen("heavy_f32", 40 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wd = np.stack([gen("heavy_f32", 50 + i, (K_OUT, HIDDEN)) for i in range(COUNT)])
    maps = [np.stack([random_map(shape, seed + i) for i in range(COUNT)]) for shape, seed in (((HIDDEN, K_IN), 33), ((HIDDEN, K_IN), 43), ((K_OUT, HIDDEN), 53))]
    assert not np.array_equal(maps[0][0], maps[0][1])
    return tuple(packed.pack_batch(torch.from_numpy(w).cuda(), m, backend="hip") for w, m in zip((wg, wu, wd), maps))


def _layer_want(x, ids, w, base, expert_dtype, out_dtype, decode_max_rows):
    """Sort on the host, the existing PackedExpertsMLP on the sorted rows with a host group_rows, the NumPy combine."""
    T, K = ids.shape
    group_rows, row_of, src = _want_plan(ids, COUNT)
    R = int(group_rows[-1])
    assert R > 0
    xg = x[torch.from_numpy(src[:R].astype(np.int64) // K).cuda()]
    mlp = packed.PackedExpertsMLP(*_experts(), out_dtype=expert_dtype, decode_max_rows=decode_max_rows)
    ys_r = mlp(xg, [int(v) for v in group_rows]).float().cpu().numpy()
    ys = np.zeros((T * K, K_OUT), dtype=np.float32)
    ys[:R] = ys_r
    with np.errstate(all="ignore"):
        acc = _want_combine(row_of, w, ys, base, T, K)
    return acc.view(np.int32) if out_dtype == "float32" else _bf16_words(acc).reshape(T, K_OUT)


def _layer_inputs(T, K, kind, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", seed, (T, K_IN)) * 50)).to(torch.bfloat16).cuda()      # unit variance
    if kind == "uniform":
        ids = rng.integers(0, COUNT, size=(T, K)).astype(np.int64)
    else:                                                 # experts 1 and 3 stay empty, some slots name experts of another rank
        ids = rng.choice(np.array([0, 2, 4, -1, COUNT, COUNT + 3], dtype=np.int64), size=(T, K))
        ids[0] = [0, -1][:K] if K <= 2 else ids[0]
        assert not np.isin(ids, (1, 3)).any() and (ids < 0).any()
    w = rng.random((T, K)).astype(np.float32) + 0.25
    base = _bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))
    return x, ids, w, base


@pytest.mark.parametrize("T,K,decode_max_rows,kind", ((37, 2, None, "uniform"), (3, 2, 64, "uniform"), (37, 2, None, "sparse"), (3, 2, 64, "sparse")))
def test_packed_moe_is_sort_experts_combine(T, K, decode_max_rows, kind):
    x, ids, w, base = _layer_inputs(T, K, kind, 7 * T + K)
    ids_d, w_d = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()
    for expert_dtype in ("float32", "bfloat16"):
        for out_dtype in ("bfloat16", "float32"):
            moe = packed.PackedMoE(*_experts(), out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=decode_max_rows)
            assert moe.backend == "hip" and (moe.count, moe.in_features, moe.out_features) == (COUNT, K_IN, K_OUT)
            for with_base in (False, True):
                want = _layer_want(x, ids, w, base if with_base else None, expert_dtype, out_dtype, decode_max_rows)
                based = torch.from_numpy(base).cuda().to(torch.bfloat16) if with_base else None
                y = moe(x, ids_d, w_d, base=based)
                assert tuple(y.shape) == (T, K_OUT) and y.dtype == (torch.float32 if out_dtype == "float32" else torch.bfloat16)
                assert np.array_equal(_bits(y), want), (expert_dtype, out_dtype, with_base, np.argwhere(_bits(y) != want)[:4])
                assert np.array_equal(_bits(moe(x, ids_d.to(torch.int32), w_d, base=based)), want), "int32 ids give other words"


@pytest.mark.filterwarnings("ignore:Synchronization debug mode is a prototype feature")
def test_packed_moe_forward_reads_nothing_back():
    """No device-to-host copy and no .item() in a forward, on either route: torch refuses the synchronising calls it knows of (those
    two among them) while the mode is "error"."""
    x, ids, w, base = _layer_inputs(37, 2, "sparse", 5)
    ids_d, w_d, based = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(base).cuda().to(torch.bfloat16)
    moe = packed.PackedMoE(*_experts(), decode_max_rows=64, max_tokens=1)
    calls = ((x, ids_d, w_d, based), (x[:3], ids_d[:3], w_d[:3], None))       # S = 74: the wide route; S = 6: the skinny one
    want = [_bits(moe(a, b, c, base=d)) for a, b, c, d in calls]               # the first calls: the workspace grows here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [moe(a, b, c, base=d) for a, b, c, d in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(np.array_equal(_bits(g), w_) for g, w_ in zip(got, want))


def test_packed_moe_keeps_leading_dimensions_and_takes_no_tokens():
    x, ids, w, _base = _layer_inputs(10, 2, "uniform", 99)
    moe = packed.PackedMoE(*_experts(), max_tokens=1)     # a workspace for one run of one token: regrown on demand, never too short
    flat = moe(x, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda())
    y = moe(x.reshape(2, 5, K_IN), torch.from_numpy(ids).cuda().reshape(2, 5, 2), torch.from_numpy(w).cuda().reshape(2, 5, 2))
    assert tuple(y.shape) == (2, 5, K_OUT) and y.dtype == torch.bfloat16
    assert np.array_equal(_bits(y).reshape(10, K_OUT), _bits(flat))
    assert np.array_equal(_bits(flat), _layer_want(x, ids, w, None, "float32", "bfloat16", None))
    empty = moe(x[:0], torch.from_numpy(ids[:0]).cuda(), torch.from_numpy(w[:0]).cuda())
    assert tuple(empty.shape) == (0, K_OUT) and empty.dtype == torch.bfloat16
    with pytest.raises(hb.MtqError, match="topk_weights must be"):
        moe(x, torch.from_numpy(ids).cuda(), torch.from_numpy(w[:, :1]).cuda())
