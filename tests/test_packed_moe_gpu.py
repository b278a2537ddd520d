"""GPU: the MoE routing kernels of csrc/mtq_moe.hip (mtq_moe_plan, mtq_moe_dispatch, mtq_moe_combine) and packed.PackedMoE on them.

The want-side is never the code under test: the plan is np.argsort(kind="stable"), the dispatch a NumPy gather, the combine a float32
NumPy loop in the contract's order (all three in tests/moe_cases.py, which the host file draws from too), and the layer is the
existing PackedExpertsMLP on a routing sorted on the host followed by that loop.  Everything is compared as integer words.  Where a
case is there for a path or a trip of a loop, the test derives that path or trip from the shape with the host code's arithmetic
(moe_cases.dispatch_geometry, combine_geometry) and asserts it.

  plan      (T, K, count) = (1, 1, 1), (1, 8, 256), (7, 2, 5), (64, 8, 256), (128, 8, 256): S = 1024, the last one-launch size,
            (129, 8, 256): the first three-kernel size, (300, 6, 300): more experts than a 256-thread block and no power of two,
            (4099, 8, 256): 33 runs, the last ragged, (16, 64, 4096): topk and count at their limits in one launch, 64 experts a lane
            in the scan, (17, 64, 4096): the same limits on three kernels, 16 experts a thread, 32 KiB of hist, (1025, 1, 1): three
            kernels with one slot a token and one expert, (256, 8, 256): two whole runs and no ragged one, (1024, 8, 64) and
            (1025, 8, 64): 8 and 9 runs, the last whole batch of the hist scan's 8 loads in flight and one past it; each with uniform
            ids, every slot on one expert, tokens that name one expert twice, about a quarter of the ids replaced by -1, count and the
            id type's minimum and maximum, no live id at all (R = 0), slot s on expert s % count (64 leaders in a 64-slot step), and
            int64 ids a multiple of 2^32 away from a live one; int32 and int64 ids; ids contiguous and as a view of a wider buffer;
            over a workspace of 0xFF bytes with sentinels behind it; twice, same words.
  dispatch  k = 8, 64, 300, 1000, 2056: 257 chunks of 16 bytes, a second trip for lane 0 alone, 4096: two whole trips; x contiguous,
            a view of a wider buffer, and starting at an unaligned element; xs a pitched view of sentinels with sentinel rows behind
            it, x with rows behind it that must not be read; a hand-made src with -1, S and the int32 extremes.
            Past the grid of 8192 workgroups: k = 129 with 8250 rows (element path, a row a workgroup), k = 520 with 16500 rows
            (16-byte path, two rows a workgroup), bad entries behind the grid's first pass.
  combine   n = 8, 72, 200, 1000, 1032: 256 lanes a token, a token a workgroup, 2056: a second trip for lane 0, 2050: the same on the
            element path with 2 ragged columns, 4096: two whole trips; ys bf16 / float32, y float32 / bf16, base none / bf16 /
            float32; weights with negative values and exact zeros; rows of ys from R on hold NaN and Inf words; a row_of with -1, S and
            the int32 extremes; y a pitched view of sentinels, at an aligned and at an odd pitch (the 16-byte and the element path).
            K = 1, 2, 3, 5, 7, 8, 9, 64 at n = 72 and n = 13: the batches of four slots, whole and ragged, with a token whose live
            slots are all in the first batch and one whose live slots are all behind it.
            Past the grid: 32800 tokens of n = 8 and n = 5 (four tokens a workgroup), 8200 tokens of n = 1032 (one).
  layer     5 experts, 128 → 96 → 64, a different random map per expert: T = 37, K = 2 on the wide route, T = 3, K = 2 with
            decode_max_rows = 64 on the skinny route, a routing that leaves two experts empty and drops slots, both expert_dtypes, with
            a base, and leading dimensions (2, 5); T = 130, K = 8: the three-kernel plan and the second combine batch inside a
            forward, then T = 3, K = 8 on the workspace that call grew; T = 4, K = 9: more slots a token than the first workspace
            was sized for.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_cases
from tests.inputs import gen, to_bf16_valued
from tests.moe_cases import (CK, CT, DK, DT, KINDS, NEVER, ROUTINGS, SENTINEL, _bf16_valued, _bf16_words, _combine_case,
                             _combine_permuted_case, _dispatch_case, _routing, _want_combine, _want_plan)      # other files import them here
from tests.packed_cases import random_map

pytestmark = pytest.mark.gpu
ID_TYPES = ((np.int32, torch.int32), (np.int64, torch.int64))


def _bits(t) -> np.ndarray:
    """The words of a device tensor: int16 for bf16, int32 for float32 and int32."""
    t = t.detach()
    return (t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)).cpu().numpy()


@pytest.mark.parametrize("T,K,count", ROUTINGS)
def test_plan_is_the_stable_sort_of_the_slots(T, K, count):
    S = T * K
    need = hb.moe_plan_workspace_bytes(T, K, count)
    assert need == ((S + 1023) // 1024 * count * 4 + 15) // 16 * 16 > 0
    assert moe_cases.RUN == hb.MOE_RUN
    runs, one_launch = (S + moe_cases.RUN - 1) // moe_cases.RUN, S <= moe_cases.RUN
    if (K, count) == (64, 4096):                          # the limits: the scan's experts per thread on either route
        assert (K, count) == (hb.MOE_MAX_TOPK, hb.MOE_MAX_EXPERTS)
        assert (runs, moe_cases.plan_scan_per(count, one_launch)) == ((1, 64) if T == 16 else (2, 16)) and (T == 16 or need == 32768)
    if (T, K, count) == (256, 8, 256):
        assert not one_launch and S % moe_cases.RUN == 0
    if count == 64:
        assert runs == (8 if T == 1024 else 9)            # the hist scan takes 8 runs a batch
    buf = torch.empty((need + 64,), dtype=torch.uint8, device="cuda")
    for kind in KINDS:
        for np_type, torch_type in ID_TYPES:
            if kind == "high_word" and np_type != np.int64:
                continue                                  # an int32 id has no high word
            ids = _routing(T, K, count, kind, np_type)
            want = _want_plan(ids, count)
            moe_cases.check_kind(kind, ids, count, want)
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

def _as_bf16(words):
    return torch.from_numpy(words.view(np.int16)).cuda().view(torch.bfloat16)


def _rows_16(*tensors) -> bool:
    """Every tensor starts 16-byte aligned and its rows are a multiple of 16 bytes apart: the operands' share of the host code's `vec`."""
    return all(t.data_ptr() % 16 == 0 and (t.stride(0) * t.element_size()) % 16 == 0 for t in tensors)


DISPATCH_TRIPS = {8: 1, 64: 1, 300: None, 1000: 1, 2056: 2, 4096: 2}         # of lane 0 on the 16-byte path; 300 has none


@pytest.mark.parametrize("k", tuple(DISPATCH_TRIPS))
def test_dispatch_copies_the_named_rows_and_zeroes_the_rest(k):
    S = DT * DK
    x, src, want = _dispatch_case(k)
    assert not (x == NEVER).any()                         # the words behind x: no output may hold them
    src_d = torch.from_numpy(src).cuda()
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), src_d, src_d, DT, DK, 1)
    behind = np.full((DT + 2, k + 8), NEVER, dtype=np.uint16)
    behind[:DT, :k] = x
    odd = np.full((DT + 2, k + 5), NEVER, dtype=np.uint16)
    odd[:DT, :k] = x
    flat = np.full((3 + (DT + 2) * k,), NEVER, dtype=np.uint16)
    flat[3: 3 + DT * k] = x.reshape(-1)
    views = {"contiguous": _as_bf16(x), "wider": _as_bf16(behind)[:DT, :k], "odd pitch": _as_bf16(odd)[:DT, :k],
             "unaligned": _as_bf16(flat)[3: 3 + DT * k].view(DT, k)}
    met = set()
    for name, xd in views.items():
        y = packed.moe_dispatch(xd, plan)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (S, k)
        assert np.array_equal(_bits(y).view(np.uint16), want), (name, k)
        vec = k % 8 == 0 and _rows_16(xd, y)              # the path this call took, by the host code's rule
        assert vec == (k % 8 == 0 and name in ("contiguous", "wider")), (name, k)
        L, _per_block, trips = moe_cases.dispatch_geometry(k, vec)
        met.add((vec, L, trips))
        for pad in (8, 3):                                # a pitched xs of sentinels with sentinel rows behind it
            out = torch.full((S + 2, k + pad), -1.0, dtype=torch.bfloat16, device="cuda")
            fill = _bits(out)[0, 0]
            y = packed.moe_dispatch(xd, plan, out=out[:S, :k])
            assert (k % 8 == 0 and _rows_16(xd, out)) == (vec and pad == 8)
            got = _bits(out)
            assert np.array_equal(got[:S, :k].view(np.uint16), want), (name, k, pad)
            assert (got[S:] == fill).all() and (got[:, k:] == fill).all(), (name, k, pad, "xs was written outside S x k")
    if DISPATCH_TRIPS[k] is None:
        assert not any(vec for vec, _L, _trips in met)
    else:                                                 # the 16-byte path at the trip count the case is there for
        assert {(L, trips) for vec, L, trips in met if vec} == {(256 if k > 1024 else moe_cases.dispatch_geometry(k, True)[0], DISPATCH_TRIPS[k])}, met
    if k == 2056:
        assert k // 8 == 256 + 1                          # the second trip holds one chunk: lane 0 alone


@pytest.mark.parametrize("k,T,K,vec,L,per_block", ((129, 2750, 3, False, 256, 1), (520, 5500, 3, True, 128, 2)))
def test_dispatch_strides_past_its_grid(k, T, K, vec, L, per_block):
    S = T * K
    assert moe_cases.dispatch_geometry(k, vec)[:2] == (L, per_block)
    first_pass = moe_cases.MAX_BLOCKS * per_block         # rows the grid's first pass covers
    assert S > first_pass
    x, src, want = _dispatch_case(k, T, K, first_pass)
    assert ((src[first_pass:] < 0) | (src[first_pass:] >= S)).sum() == 2
    src_d, xd = torch.from_numpy(src).cuda(), _as_bf16(x)
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), src_d, src_d, T, K, 1)
    out = torch.full((S + 2, k + (8 if vec else 3)), -1.0, dtype=torch.bfloat16, device="cuda")
    fill = _bits(out)[0, 0]
    packed.moe_dispatch(xd, plan, out=out[:S, :k])
    assert (k % 8 == 0 and _rows_16(xd, out)) == vec
    got = _bits(out)
    wrong = np.flatnonzero((got[:S, :k].view(np.uint16) != want).any(axis=1))
    assert wrong.size == 0, (k, "rows", wrong[:8], "of them past the first pass", int((wrong >= first_pass).sum()))
    assert (got[S:] == fill).all() and (got[:, k:] == fill).all(), (k, "xs was written outside S x k")


# ----------------------------------------------------------------------------- combine

def _check_combine(n, T, K, case, base_types, ys_types=(torch.bfloat16, torch.float32)):
    """The words of moe_combine against _want_combine over ys types, base types, both outputs, and y contiguous, at an aligned pitch
    (the 16-byte path when n is a multiple of 8) and at an odd one (the element path), sentinels around it."""
    S = T * K
    row_of, w, ys, ys_dev, base = case
    row_d, w_d = torch.from_numpy(row_of).cuda(), torch.from_numpy(w).cuda()
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), row_d, row_d, T, K, 1)
    wants = {None: _want_combine(row_of, w, ys, None, T, K), "base": _want_combine(row_of, w, ys, base, T, K)}
    assert not np.array_equal(wants[None], wants["base"])
    for ys_type in ys_types:
        ysd = torch.from_numpy(ys_dev).cuda().to(ys_type)                    # exact: bf16 values (NaN and Inf words stay NaN and Inf)
        for base_type in base_types:
            based = None if base_type is None else torch.from_numpy(base).cuda().to(base_type)
            want32 = wants[None if base_type is None else "base"]
            for out_dtype, torch_out in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
                want = want32.view(np.int32) if out_dtype == "float32" else _bf16_words(want32).reshape(T, n)
                what = (n, K, ys_type, base_type, out_dtype)
                y = packed.moe_combine(ysd, w_d, plan, base=based, out_dtype=out_dtype)
                assert y.dtype == torch_out and tuple(y.shape) == (T, n)
                assert np.array_equal(_bits(y), want), (what, np.argwhere(_bits(y) != want)[:4])
                for pad in (8, 3):                        # pitched y of sentinels: the 16-byte path and the element path
                    out = torch.full((T + 2, n + pad), -3.0, dtype=torch_out, device="cuda")
                    fill = _bits(out)[0, 0]
                    packed.moe_combine(ysd, w_d, plan, base=based, out_dtype=out_dtype, out=out[:T, :n])
                    vec = n % 8 == 0 and _rows_16(ysd, out, *(() if based is None else (based,)))      # the host code's rule
                    assert vec == (n % 8 == 0 and pad == 8), (what, pad)
                    got = _bits(out)
                    assert np.array_equal(got[:T, :n], want), (what, pad, np.argwhere(got[:T, :n] != want)[:4])
                    assert (got[T:] == fill).all() and (got[:, n:] == fill).all(), (what, pad, "y was written outside tokens x n")
    return plan, w_d, wants


COMBINE_MEETS = {8: (64, 4, 1), 72: (64, 4, 1), 200: (64, 4, 1), 1000: (128, 2, 1), 1032: (256, 1, 1), 2056: (256, 1, 2),
                 2050: (256, 1, 2), 4096: (256, 1, 2)}    # n: (lanes a token, tokens a workgroup, trips of lane 0 over the columns)


@pytest.mark.parametrize("n", tuple(COMBINE_MEETS))
def test_combine_sums_in_slot_order_and_skips_what_is_no_row(n):
    S = CT * CK
    assert moe_cases.combine_geometry(n) == COMBINE_MEETS[n]
    if n in (2056, 2050):
        assert (n + 7) // 8 == 256 + 1 and n - 256 * 8 == (8 if n == 2056 else 2)         # the second trip: lane 0 alone, 8 or 2 columns
    case = _combine_case(n)
    plan, w_d, wants = _check_combine(n, CT, CK, case, (None, torch.bfloat16, torch.float32))
    for ys_type in (torch.bfloat16, torch.float32):
        # operands at odd pitches and an unaligned start: the element path, the same words
        wide = torch.zeros((S, n + 3), dtype=ys_type, device="cuda")
        wide[:, :n] = torch.from_numpy(case[3]).cuda().to(ys_type)
        wpitch = torch.zeros((CT, CK + 1), dtype=torch.float32, device="cuda")
        wpitch[:, :CK] = w_d
        assert not _rows_16(wide)
        y = packed.moe_combine(wide[:, :n], wpitch[:, :CK], plan, out_dtype="float32")
        assert np.array_equal(_bits(y), wants[None].view(np.int32)), (n, ys_type, "odd pitches")


@pytest.mark.parametrize("n", (72, 13))
@pytest.mark.parametrize("K", (1, 2, 3, 5, 7, 8, 9, 64))
def test_combine_at_every_topk(K, n):
    """The slots go through the kernel four at a time: K below, at and above one batch, whole batches and ragged ones, the limit.
    n = 72: the 16-byte path; n = 13: the element path, 5 columns in the last lane's 8."""
    batches, ragged = -(-K // 4), K % 4
    assert (batches, ragged) == {1: (1, 1), 2: (1, 2), 3: (1, 3), 5: (2, 1), 7: (2, 3), 8: (2, 0), 9: (3, 1), 64: (16, 0)}[K]
    assert K <= hb.MOE_MAX_TOPK and moe_cases.combine_geometry(n)[0] == 64 and (n % 8 == 0 or n % 8 == 5)
    _check_combine(n, CT, K, _combine_case(n, K), (None, torch.bfloat16))      # at K >= 5 the case holds a token for either batch alone


@pytest.mark.parametrize("n,T,K,per_block,ys_types", ((8, 32800, 1, 4, (torch.bfloat16, torch.float32)),
                                                      (5, 32800, 1, 4, (torch.bfloat16, torch.float32)),
                                                      (1032, 8200, 2, 1, (torch.bfloat16,))))
def test_combine_strides_past_its_grid(n, T, K, per_block, ys_types):
    S = T * K
    assert moe_cases.combine_geometry(n)[1] == per_block
    first_pass = moe_cases.MAX_BLOCKS * per_block         # tokens the grid's first pass covers
    assert T > first_pass
    row_of, w, ys, base = _combine_permuted_case(n, T, K, first_pass)
    far = row_of[first_pass * K:]
    assert ((far < 0) | (far >= S)).sum() == 3            # bad entries on the tokens of the second pass
    want32 = _want_combine(row_of, w, ys, base, T, K)
    row_d, w_d = torch.from_numpy(row_of).cuda(), torch.from_numpy(w).cuda()
    plan = packed.MoEPlan(torch.zeros((2,), dtype=torch.int32, device="cuda"), row_d, row_d, T, K, 1)
    based = torch.from_numpy(base).cuda().to(torch.bfloat16)
    for ys_type in ys_types:
        ysd = torch.from_numpy(ys).cuda().to(ys_type)
        for out_dtype, torch_out in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            want = want32.view(np.int32) if out_dtype == "float32" else _bf16_words(want32).reshape(T, n)
            out = torch.full((T + 2, n + (8 if n % 8 == 0 else 3)), -3.0, dtype=torch_out, device="cuda")
            fill = _bits(out)[0, 0]
            packed.moe_combine(ysd, w_d, plan, base=based, out_dtype=out_dtype, out=out[:T, :n])
            assert (n % 8 == 0 and _rows_16(ysd, out, based)) == (n % 8 == 0)
            got = _bits(out)
            wrong = np.flatnonzero((got[:T, :n] != want).any(axis=1))
            assert wrong.size == 0, (n, ys_type, out_dtype, "tokens", wrong[:8], "of them past the first pass", int((wrong >= first_pass).sum()))
            assert (got[T:] == fill).all() and (got[:, n:] == fill).all(), (n, out_dtype, "y was written outside tokens x n")


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


@pytest.mark.parametrize("kind", ("uniform", "sparse"))
def test_packed_moe_above_one_run_then_a_small_call_on_the_grown_workspace(kind):
    """T = 130, K = 8: S = 1040, so the three-kernel plan runs inside a forward, the combine takes two batches of slots, and with 5
    experts every token names one more than once.  The module starts with a workspace for one run; the large call regrows it, and
    the T = 3 call that follows (S = 24: the one-launch plan, the skinny route) finds the large call's histogram in it and must give
    the words of a module that never made the large call."""
    T, K, small = 130, 8, 3
    assert T * K > hb.MOE_RUN and small * K <= 64 and K > 4 and K > COUNT
    x, ids, w, base = _layer_inputs(T, K, kind, 7 * T + K)
    xs, idss, ws, bases = _layer_inputs(small, K, kind, 11)
    assert (np.sort(ids, axis=1)[:, 1:] == np.sort(ids, axis=1)[:, :-1]).any(axis=1).all()
    first, grown = hb.moe_plan_workspace_bytes(1, packed.MOE_PLAN_TOPK, COUNT), hb.moe_plan_workspace_bytes(T, K, COUNT)
    assert hb.moe_plan_workspace_bytes(small, K, COUNT) <= first < grown

    def dev(ids, w, base):
        return torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(base).cuda().to(torch.bfloat16)

    (ids_d, w_d, base_d), (idss_d, ws_d, bases_d) = dev(ids, w, base), dev(idss, ws, bases)
    for expert_dtype in ("float32", "bfloat16"):
        for out_dtype in ("bfloat16", "float32"):
            moe = packed.PackedMoE(*_experts(), out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=64, max_tokens=1)
            assert moe._plan_workspace.numel() == first
            for with_base in (False, True):
                want = _layer_want(x, ids, w, base if with_base else None, expert_dtype, out_dtype, 64)
                y = moe(x, ids_d, w_d, base=base_d if with_base else None)
                assert np.array_equal(_bits(y), want), (expert_dtype, out_dtype, with_base, np.argwhere(_bits(y) != want)[:4])
            assert moe._plan_workspace.numel() == grown
            held = moe._plan_workspace.data_ptr()
            fresh = packed.PackedMoE(*_experts(), out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=64, max_tokens=1)
            for with_base in (False, True):
                want = _layer_want(xs, idss, ws, bases if with_base else None, expert_dtype, out_dtype, 64)
                y = moe(xs, idss_d, ws_d, base=bases_d if with_base else None)
                assert np.array_equal(_bits(y), want), (expert_dtype, out_dtype, with_base, "small call after the large one")
                assert np.array_equal(_bits(fresh(xs, idss_d, ws_d, base=bases_d if with_base else None)), want)
            assert moe._plan_workspace.data_ptr() == held and fresh._plan_workspace.numel() == first


def test_packed_moe_with_more_slots_a_token_than_its_workspace_was_sized_for():
    """T = 4, K = 9 on a max_tokens = 1 module: K > MOE_PLAN_TOPK, three batches of slots in the combine.  The bytes a call needs go
    by ceil(T * K / 1024) runs, so with 5 experts this call still fits the first workspace; the need is checked per call all the same."""
    T, K = 4, 9
    assert K > packed.MOE_PLAN_TOPK
    x, ids, w, base = _layer_inputs(T, K, "uniform", 7 * T + K)
    w_d, base_d = torch.from_numpy(w).cuda(), torch.from_numpy(base).cuda().to(torch.bfloat16)
    for kind_ids in (ids, np.where(np.arange(K) % 3 == 1, -1, ids)):                      # and with slots 1, 4, 7 of every token dropped
        ids_d = torch.from_numpy(np.ascontiguousarray(kind_ids)).cuda()
        for expert_dtype in ("float32", "bfloat16"):
            moe = packed.PackedMoE(*_experts(), out_dtype="float32", expert_dtype=expert_dtype, max_tokens=1)
            assert moe._plan_workspace.numel() >= hb.moe_plan_workspace_bytes(T, K, COUNT)
            for based, b in ((None, None), (base_d, base)):
                want = _layer_want(x, np.ascontiguousarray(kind_ids), w, b, expert_dtype, "float32", None)
                assert np.array_equal(_bits(moe(x, ids_d, w_d, base=based)), want), (expert_dtype, b is None)


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
