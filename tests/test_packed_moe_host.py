"""CPU-only: the MoE routing entries (packed.moe_plan, moe_dispatch, moe_combine, PackedMoE; mtq_moe_plan, mtq_moe_dispatch,
mtq_moe_combine and the plan's size function) as far as they go without a device.  The emulation backend against a plain Python loop
over the slots; the plan's invariants; every argument error; the C entries' refusals, which come back before a device is looked for
(the pointers handed in are host addresses that no check may dereference); the size function's formula; PackedMoE on the emulation
against sort on the host, PackedExpertsMLP(backend="emulation") and the combine on the host.

The table of tests/test_packed_moe_gpu.py (tests/moe_cases.py) runs here too, on the emulation and against this file's own loops, so
that the cases and the want-side the GPU file compares with are checked on a machine without a GPU:
  plan      every (T, K, count) of moe_cases.ROUTINGS with every kind of moe_cases.KINDS, both id types;
  dispatch  k = 8, 64, 300, 1000, 2056, 4096 with 111 rows; the strided grids' k = 129 and k = 520 at a tenth of their rows;
  combine   n = 8, 72, 200, 1000, 1032, 2056, 2050, 4096 at K = 4; K = 1, 2, 3, 5, 7, 8, 9, 64 at n = 72 and n = 13; the strided
            grids' permuted cases at a tenth of their tokens;
  layer     T = 130, K = 8, then T = 3, K = 8 on the same module; T = 4, K = 9."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_cases
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _OnDevice, _StubLibrary

HEADER = Path(__file__).resolve().parents[1] / "include" / "mtq.h"
NEW = ("mtq_moe_plan_workspace_bytes", "mtq_moe_plan", "mtq_moe_dispatch", "mtq_moe_combine")
INVALID, NO_DEVICE = -1, -3
BAD_SIZE = 2 ** 64 - 1
ROUTINGS = ((1, 1, 1), (1, 8, 256), (7, 2, 5), (64, 8, 256), (128, 8, 256), (129, 8, 256), (300, 6, 300), (4099, 8, 256))
KINDS = ("uniform", "one", "twice", "dropped")


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def _routing(T, K, count, kind, np_type=np.int64):
    rng = np.random.default_rng(1000 * T + 10 * K + count)
    ids = rng.integers(0, count, size=(T, K)).astype(np_type)
    if kind == "one":
        ids[:] = count // 2
    elif kind == "twice" and K > 1:
        ids[:, -1] = ids[:, 0]
    elif kind == "dropped":
        info = np.iinfo(np_type)
        bad = np.array([-1, count, info.min, info.max], dtype=np_type)
        drop = rng.random((T, K)) < 0.25
        drop.reshape(-1)[-1] = True
        ids[drop] = bad[rng.integers(0, 4, size=int(drop.sum()))]
    return ids


def _loop_plan(ids, count):
    """The contract, slot by slot: a counting pass, the prefix, then the slots in ascending order take their expert's next row."""
    flat = [int(v) for v in ids.reshape(-1)]
    per = [0] * count
    for e in flat:
        if 0 <= e < count:
            per[e] += 1
    group_rows = [0]
    for c in per:
        group_rows.append(group_rows[-1] + c)
    nxt, row_of, src = list(group_rows[:-1]), [-1] * len(flat), [-1] * len(flat)
    for s, e in enumerate(flat):
        if 0 <= e < count:
            row_of[s] = nxt[e]
            src[nxt[e]] = s
            nxt[e] += 1
    return np.array(group_rows, dtype=np.int32), np.array(row_of, dtype=np.int32), np.array(src, dtype=np.int32)


def test_the_entries_are_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name) is not None
    assert set(hb.MOE) == set(NEW) and hb.has_moe() is True
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    for const, value in (("MTQ_MOE_MAX_TOPK", hb.MOE_MAX_TOPK), ("MTQ_MOE_MAX_EXPERTS", hb.MOE_MAX_EXPERTS), ("MTQ_MOE_RUN", hb.MOE_RUN)):
        assert re.search(rf"#define {const} {value}\b", text), const
    assert (packed.MOE_MAX_TOPK, packed.MOE_MAX_EXPERTS) == (hb.MOE_MAX_TOPK, hb.MOE_MAX_EXPERTS) == (64, 4096)
    assert packed.PackedMoE is packed.PackedMoE and issubclass(packed.PackedMoE, torch.nn.Module)


def test_a_build_without_the_entries_still_loads_and_nothing_stands_in(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_skinny_grouped.argtypes is not None               # every other symbol is bound
    assert hb.has_packed_glu_skinny() and not hb.has_moe()
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    ids = _routing(7, 2, 5, "uniform")
    with pytest.raises(hb.MtqError, match="mtq_moe_plan.*lacks.*rebuild it from this tree"):
        packed.moe_plan(ids, 5, backend="hip")
    dev = _OnDevice(torch.zeros((6,), dtype=torch.int32))
    plan = packed.MoEPlan(dev, dev, dev, 7, 2, 5)
    with pytest.raises(hb.MtqError, match="mtq_moe_plan.*lacks.*rebuild it from this tree"):
        packed.moe_dispatch(torch.zeros((7, 8), dtype=torch.bfloat16), plan)
    with pytest.raises(hb.MtqError, match="mtq_moe_plan.*lacks.*rebuild it from this tree"):
        packed.moe_combine(torch.zeros((14, 8)), np.zeros((7, 2), dtype=np.float32), plan)


def test_the_size_function_gives_the_formula_and_never_zero():
    fn = hb._entry(NEW[0])
    for T, K, count in ROUTINGS + ((1024, 1, 4096), (1025, 1, 1), (33, 64, 3), (2 ** 31 - 1, 1, 1), ((2 ** 31 - 1) // 64, 64, 4096)):
        want = ((T * K + 1023) // 1024 * count * 4 + 15) // 16 * 16
        assert hb.moe_plan_workspace_bytes(T, K, count) == fn(T, K, count) == want > 0, (T, K, count)
    assert hb.moe_plan_workspace_bytes(1, 1, 1) == 16 and hb.moe_plan_workspace_bytes(1025, 8, 5) == 192
    for bad in ((0, 8, 256), (-1, 8, 256), (7, 0, 5), (7, 65, 5), (7, -2, 5), (7, 2, 0), (7, 2, 4097), (7, 2, -1), (2 ** 31, 1, 1),
                (2 ** 30, 2, 1), (2 ** 62, 64, 1)):
        assert fn(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.moe_plan_workspace_bytes(*bad)


def test_plan_refuses_before_a_device():
    fn = hb._entry(NEW[1])
    _buf, p = _aligned()
    T, K, count = 300, 6, 300
    need = hb.moe_plan_workspace_bytes(T, K, count)

    def call(ids=p, dtype=hb.IDS_I64, ld=K, T=T, K=K, count=count, rows=p, row_of=p, src=p, ws=p, ws_bytes=1 << 15):
        return fn(ids, dtype, ld, T, K, count, rows, row_of, src, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("ids", "rows", "row_of", "src"):
        refused("null argument", **{name: None})
    refused("id_dtype", dtype=2)
    refused("id_dtype", dtype=-1)
    refused("tokens must be positive", T=0)
    refused("topk must be", K=0, ld=1)
    refused("topk must be", K=65, ld=65)
    refused("count must be", count=0)
    refused("count must be", count=4097)
    refused("below 2^31", T=2 ** 31 // 6 + 1)
    refused("ld_ids < topk", ld=K - 1)
    refused("aligned to its type", ids=p + 4)
    refused("4-byte aligned", src=p + 2)
    refused("workspace is null", ws=None)
    refused("workspace is null", ws=None, ws_bytes=0)
    refused("workspace must be 16-byte aligned", ws=p + 8)
    refused("smaller than the", ws_bytes=need - 1)
    refused("smaller than the", ws_bytes=0)
    refused("workspace is null", T=1, K=1, ld=1, count=1, ws=None)              # the one-launch sizes take one all the same
    refused("smaller than the", T=1, K=1, ld=1, count=1, ws_bytes=15)
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert call() == NO_DEVICE and call(ws_bytes=need) == NO_DEVICE and call(dtype=hb.IDS_I32, ids=p + 4, ld=K + 3) == NO_DEVICE
        assert call(T=1, K=1, ld=1, count=1, ws_bytes=16) == NO_DEVICE


def test_dispatch_refuses_before_a_device():
    fn = hb._entry(NEW[2])
    _buf, p = _aligned()

    def call(x=p, T=7, k=40, ldx=40, src=p, K=2, xs=p, ldxs=40):
        return fn(x, T, k, ldx, src, K, xs, ldxs, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "src", "xs"):
        refused("null argument", **{name: None})
    refused("tokens must be positive", T=0)
    refused("topk must be", K=0)
    refused("topk must be", K=65)
    refused("below 2^31", T=2 ** 30)
    refused("k must be positive", k=0)
    refused("matrix too large", k=2 ** 30 + 1, ldx=2 ** 31, ldxs=2 ** 31)
    refused("ldx < k", ldx=39)
    refused("ldxs < k", ldxs=39)
    refused("not aligned to its type", x=p + 1)
    refused("not aligned to its type", src=p + 2)
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(x=p + 2, ldx=41, ldxs=47) == NO_DEVICE


def test_combine_refuses_before_a_device():
    fn = hb._entry(NEW[3])
    _buf, p = _aligned()

    def call(ys=p, ys_dtype=hb.DTYPE_BF16, ldys=40, row_of=p, w=p, ldw=2, base=None, base_dtype=0, ldbase=0, T=7, K=2, n=40, y=p,
             out_dtype=hb.DTYPE_F32, ldy=40):
        return fn(ys, ys_dtype, ldys, row_of, w, ldw, base, base_dtype, ldbase, T, K, n, y, out_dtype, ldy, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("ys", "row_of", "w", "y"):
        refused("null argument", **{name: None})
    refused("ys_dtype", ys_dtype=2)
    refused("out_dtype", out_dtype=7)
    refused("base_dtype", base=p, base_dtype=3, ldbase=40)
    refused("tokens must be positive", T=-1)
    refused("topk must be", K=65, ldw=65)
    refused("n must be positive", n=0)
    refused("ldys < n", ldys=39)
    refused("ldw < topk", ldw=1)
    refused("ldbase < n", base=p, ldbase=39)
    refused("ldy < n", ldy=39)
    refused("not aligned to its type", ys_dtype=hb.DTYPE_F32, ys=p + 2)
    refused("not aligned to its type", y=p + 2)
    refused("not aligned to its type", base=p + 1, ldbase=40)
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(base=p + 2, ldbase=41, ys=p + 4, ys_dtype=hb.DTYPE_F32, out_dtype=hb.DTYPE_BF16, y=p + 2) == NO_DEVICE
        assert call(base_dtype=9, ldbase=-5) == NO_DEVICE                        # without a base they mean nothing


def test_the_bindings_check_their_operands_before_a_device():
    ids = _OnDevice(torch.zeros((7, 2), dtype=torch.int64))
    with pytest.raises(hb.MtqError, match="2-D"):
        hb.moe_plan(_OnDevice(torch.zeros((7,), dtype=torch.int64)), 5)
    with pytest.raises(hb.MtqError, match="int32 or int64"):
        hb.moe_plan(_OnDevice(torch.zeros((7, 2))), 5)
    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.moe_plan(_OnDevice(torch.zeros((7, 4), dtype=torch.int64)[:, ::2]), 5)
    with pytest.raises(hb.MtqError, match="device tensor"):
        hb.moe_plan(torch.zeros((7, 2), dtype=torch.int64), 5)
    with pytest.raises(hb.MtqError, match="count must be"):
        hb.moe_plan(ids, 0)
    x = _OnDevice(torch.zeros((7, 40), dtype=torch.bfloat16))
    src = _OnDevice(torch.zeros((14,), dtype=torch.int32))
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.moe_dispatch(_OnDevice(torch.zeros((7, 40))), src, 2)
    with pytest.raises(hb.MtqError, match="src must"):
        hb.moe_dispatch(x, _OnDevice(torch.zeros((13,), dtype=torch.int32)), 2)
    with pytest.raises(hb.MtqError, match=r"tokens \* topk = 14"):
        hb.moe_dispatch(x, _OnDevice(torch.zeros((15,), dtype=torch.int32)), 2)
    with pytest.raises(hb.MtqError, match=r"out must be a torch.bfloat16 \(14, 40\)"):
        hb.moe_dispatch(x, src, 2, out=_OnDevice(torch.zeros((14, 40))))
    w = _OnDevice(torch.zeros((7, 2)))
    ys = _OnDevice(torch.zeros((14, 40), dtype=torch.bfloat16))
    with pytest.raises(hb.MtqError, match="weights must be a float32"):
        hb.moe_combine(ys, src, _OnDevice(torch.zeros((7, 2), dtype=torch.bfloat16)))
    with pytest.raises(hb.MtqError, match=r"ys must be \(14, n\)"):
        hb.moe_combine(_OnDevice(torch.zeros((13, 40))), src, w)
    with pytest.raises(hb.MtqError, match="row_of must"):
        hb.moe_combine(ys, _OnDevice(torch.zeros((14,), dtype=torch.int64)), w)
    with pytest.raises(hb.MtqError, match=r"base must be \(7, 40\)"):
        hb.moe_combine(ys, src, w, base=_OnDevice(torch.zeros((7, 41))))
    with pytest.raises(hb.MtqError, match="output type"):
        hb.moe_combine(ys, src, w, out_dtype=torch.float16)


# ----------------------------------------------------------------------------- the emulation

@pytest.mark.parametrize("T,K,count", ROUTINGS)
def test_the_emulated_plan_is_the_loop_over_the_slots(T, K, count):
    S = T * K
    for kind in KINDS:
        for np_type in (np.int32, np.int64):
            ids = _routing(T, K, count, kind, np_type)
            want = _loop_plan(ids, count)
            for given in (ids, torch.from_numpy(ids)):
                plan = packed.moe_plan(given, count)
                assert not plan.on_device and (plan.tokens, plan.topk, plan.count, plan.slots) == (T, K, count, S)
                for got, w, name in zip((plan.group_rows, plan.row_of, plan.src), want, ("group_rows", "row_of", "src")):
                    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, w), (kind, name)
            # the invariants, stated on their own
            g, row_of, src = plan.group_rows, plan.row_of, plan.src
            R = int(g[-1])
            live = np.flatnonzero(row_of >= 0)
            assert g[0] == 0 and (np.diff(g) >= 0).all() and R == live.size <= S
            assert np.array_equal(src[row_of[live]], live) and (src[R:] == -1).all() and (src[:R] >= 0).all()
            flat = ids.astype(np.int64).reshape(-1)
            assert np.array_equal(live, np.flatnonzero((flat >= 0) & (flat < count)))
            assert (np.diff(flat[src[:R]]) >= 0).all()                                    # expert order
            same = np.diff(flat[src[:R]]) == 0
            assert (np.diff(src[:R])[same] > 0).all()                                     # stable inside an expert
            if kind == "twice" and K > 1:
                assert (row_of.reshape(T, K)[:, 0] != row_of.reshape(T, K)[:, -1]).all()  # one expert twice: a row each


def test_the_emulated_dispatch_and_combine_are_the_loops():
    T, K, count, k = 19, 4, 6, 24
    ids = _routing(T, K, count, "dropped")
    plan = packed.moe_plan(ids, count)
    S, R = plan.slots, int(plan.group_rows[-1])
    assert 0 < R < S
    x = to_bf16_valued(gen("normal_f32", 3, (T, k)) * 50)
    want = np.zeros((S, k), dtype=np.float32)
    for r in range(S):
        if 0 <= plan.src[r] < S:
            want[r] = x[plan.src[r] // K]
    xs = packed.moe_dispatch(x, plan)
    assert isinstance(xs, np.ndarray) and np.array_equal(xs.view(np.uint32), want.view(np.uint32))
    xt = packed.moe_dispatch(torch.from_numpy(x).to(torch.bfloat16), plan)
    assert xt.dtype == torch.bfloat16 and torch.equal(xt.float(), torch.from_numpy(want)) and not xt[R:].any()
    # a hand-made src: what is no slot gives a zero row
    odd = packed.MoEPlan(plan.group_rows, plan.row_of, np.array([-1, S, -2 ** 31, 2 ** 31 - 1] + [5] * (S - 4), dtype=np.int32), T, K, count)
    xo = packed.moe_dispatch(x, odd)
    assert not xo[:4].any() and np.array_equal(xo[4:], np.broadcast_to(x[5 // K], (S - 4, k)))

    rng = np.random.default_rng(5)
    w = rng.standard_normal((T, K)).astype(np.float32)
    w[rng.random((T, K)) < 0.2] = 0.0
    ys = to_bf16_valued(rng.standard_normal((S, k)).astype(np.float32) * 3)
    ys[R:] = np.inf                                       # never read
    base = to_bf16_valued(rng.standard_normal((T, k)).astype(np.float32))
    row_of = plan.row_of.copy()
    row_of[np.flatnonzero(row_of >= 0)[[0, 3]]] = [S, -2 ** 31]
    hand = packed.MoEPlan(plan.group_rows, row_of, plan.src, T, K, count)
    for b in (None, base):
        acc = np.zeros((T, k), dtype=np.float32) if b is None else b.copy()
        for t in range(T):
            for j in range(K):
                r = int(row_of[t * K + j])
                if 0 <= r < S:
                    for c in range(k):
                        acc[t, c] = np.float32(acc[t, c] + np.float32(w[t, j] * ys[r, c]))
        assert np.isfinite(acc).all()
        y = packed.moe_combine(ys, w, hand, base=b)
        assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), acc.view(np.uint32))
        for given in (torch.from_numpy(ys), torch.from_numpy(ys).to(torch.bfloat16)):
            bt = None if b is None else torch.from_numpy(b).to(torch.bfloat16)
            yb = packed.moe_combine(given, torch.from_numpy(w), hand, base=bt, out_dtype="bfloat16")
            assert yb.dtype == torch.bfloat16 and torch.equal(yb.view(torch.int16), torch.from_numpy(acc).to(torch.bfloat16).view(torch.int16))


# ----------------------------------------------------------------------------- the GPU file's table (tests/moe_cases.py) on the emulation

def _loop_dispatch(x, src, K):
    S = src.size
    want = np.zeros((S, x.shape[1]), dtype=x.dtype)
    for r in range(S):
        if 0 <= src[r] < S:
            want[r] = x[src[r] // K]
    return want


def _loop_combine(row_of, w, ys, base, T, K):
    """The contract, slot by slot: acc = fl32(acc + fl32(w * ys[row])) with the two roundings as two NumPy float32 operations."""
    S = T * K
    acc = np.zeros((T, ys.shape[1]), dtype=np.float32) if base is None else np.array(base, dtype=np.float32)
    for s in range(S):
        r = int(row_of[s])
        if 0 <= r < S:
            product = np.multiply(w[s // K, s % K], ys[r], dtype=np.float32)
            np.add(acc[s // K], product, out=acc[s // K], dtype=np.float32)
    assert np.isfinite(acc).all()
    return acc


@pytest.mark.parametrize("T,K,count", moe_cases.ROUTINGS)
def test_the_shared_routings_on_the_emulation_and_their_want_side(T, K, count):
    """Every (T, K, count) and kind of the GPU file: the emulated plan and the want-side the GPU file compares with (moe_cases._want_plan)
    against this file's loop, and what each kind promises (moe_cases.check_kind)."""
    for kind in moe_cases.KINDS:
        for np_type in (np.int32, np.int64):
            if kind == "high_word" and np_type != np.int64:
                continue
            ids = moe_cases._routing(T, K, count, kind, np_type)
            want = _loop_plan(ids, count)
            moe_cases.check_kind(kind, ids, count, want)
            plan = packed.moe_plan(ids, count)
            for got, shared, w, name in zip((plan.group_rows, plan.row_of, plan.src), moe_cases._want_plan(ids, count), want,
                                            ("group_rows", "row_of", "src")):
                assert got.dtype == shared.dtype == np.int32 and np.array_equal(got, w) and np.array_equal(shared, w), (kind, name)
            if kind == "none_live":
                assert int(plan.group_rows[-1]) == 0
            if (T, K, count) == (1025, 1, 1) and kind in ("uniform", "one", "twice", "distinct"):
                assert np.array_equal(plan.row_of, np.arange(T))                           # every slot's row is its own index


@pytest.mark.parametrize("k,T,K,far", tuple((k, moe_cases.DT, moe_cases.DK, None) for k in (8, 64, 300, 1000, 2056, 4096)) +
                         ((129, 275, 3, 700), (520, 550, 3, 1500)))                       # the strided grids' cases at a tenth of the rows
def test_the_shared_dispatch_cases_on_the_emulation(k, T, K, far):
    x, src, want = moe_cases._dispatch_case(k, T, K, far)
    assert np.array_equal(want, _loop_dispatch(x, src, K))
    plan = packed.MoEPlan(np.zeros(2, dtype=np.int32), src, src, T, K, 1)
    xs = packed.moe_dispatch(x.view(np.int16), plan)      # a bit copy: any 16-bit words
    assert xs.dtype == np.int16 and np.array_equal(xs.view(np.uint16), want)
    xt = packed.moe_dispatch(torch.from_numpy(x.view(np.int16)).view(torch.bfloat16), plan)
    assert xt.dtype == torch.bfloat16 and np.array_equal(xt.view(torch.int16).numpy().view(np.uint16), want)


def _emulated_combine_is_the_loop(row_of, w, ys, ys_given, base, T, K):
    plan = packed.MoEPlan(np.zeros(2, dtype=np.int32), row_of, row_of, T, K, 1)
    for b in (None, base):
        want = _loop_combine(row_of, w, ys, b, T, K)
        assert np.array_equal(moe_cases._want_combine(row_of, w, ys, b, T, K).view(np.int32), want.view(np.int32))    # the GPU file's want
        y = packed.moe_combine(ys_given, w, plan, base=b)
        assert y.dtype == np.float32 and np.array_equal(y.view(np.int32), want.view(np.int32)), (T, K, ys.shape[1], b is None)
        bt = None if b is None else torch.from_numpy(b).to(torch.bfloat16)
        yb = packed.moe_combine(torch.from_numpy(ys_given).to(torch.bfloat16), torch.from_numpy(w), plan, base=bt, out_dtype="bfloat16")
        assert yb.dtype == torch.bfloat16 and np.array_equal(yb.view(torch.int16).numpy(), moe_cases._bf16_words(want).reshape(T, -1))


@pytest.mark.parametrize("n,K", tuple((n, moe_cases.CK) for n in (8, 72, 200, 1000, 1032, 2056, 2050, 4096)) +
                         tuple((n, K) for n in (72, 13) for K in (1, 2, 3, 5, 7, 8, 9, 64)))
def test_the_shared_combine_cases_on_the_emulation(n, K):
    row_of, w, ys, ys_dev, base = moe_cases._combine_case(n, K)
    _emulated_combine_is_the_loop(row_of, w, ys, ys_dev, base, moe_cases.CT, K)           # ys_dev: NaN and Inf in the rows no slot names


@pytest.mark.parametrize("n,T,K", ((8, 3280, 1), (5, 3280, 1), (1032, 820, 2)))           # the strided grids' cases at a tenth of the tokens
def test_the_shared_permuted_combine_cases_on_the_emulation(n, T, K):
    row_of, w, ys, base = moe_cases._combine_permuted_case(n, T, K, T - 8)
    _emulated_combine_is_the_loop(row_of, w, ys, ys, base, T, K)


def test_the_launch_geometry_the_gpu_tests_assert():
    """moe_cases' copy of the host code's arithmetic at the sizes the GPU file claims: which k and n take a second trip, which n take
    256 lanes, and how many rows a workgroup holds where the grids stride."""
    assert [moe_cases.dispatch_geometry(k, True) for k in (8, 1000, 2048, 2056, 4096)] == [(1, 256, 1), (128, 2, 1), (256, 1, 1), (256, 1, 2), (256, 1, 2)]
    assert moe_cases.dispatch_geometry(129, False) == (256, 1, 1) and moe_cases.dispatch_geometry(520, True) == (128, 2, 1)
    assert [moe_cases.combine_geometry(n) for n in (5, 8, 13, 72, 1000, 1024, 1032, 2048, 2050, 2056, 4096)] == \
        [(64, 4, 1)] * 4 + [(128, 2, 1), (128, 2, 1), (256, 1, 1), (256, 1, 1), (256, 1, 2), (256, 1, 2), (256, 1, 2)]
    assert 2750 * 3 > moe_cases.MAX_BLOCKS * 1 and 5500 * 3 > moe_cases.MAX_BLOCKS * 2 and 32800 > moe_cases.MAX_BLOCKS * 4 and 8200 > moe_cases.MAX_BLOCKS
    assert (moe_cases.plan_scan_per(4096, True), moe_cases.plan_scan_per(4096, False)) == (64, 16) and moe_cases.RUN == hb.MOE_RUN


def test_every_argument_error():
    ids = _routing(7, 2, 5, "uniform")
    for bad in (ids.reshape(-1), ids.reshape(7, 2, 1), torch.from_numpy(ids)[0]):
        with pytest.raises(hb.MtqError, match="2-D"):
            packed.moe_plan(bad, 5)
    for bad in (ids.astype(np.float32), torch.from_numpy(ids).float(), ids.astype(np.int16)):
        with pytest.raises(hb.MtqError, match="int32 or int64"):
            packed.moe_plan(bad, 5)
    with pytest.raises(hb.MtqError, match="topk must be 1 .. 64, got 65"):
        packed.moe_plan(np.zeros((3, 65), dtype=np.int64), 5)
    with pytest.raises(hb.MtqError, match="at least one token"):
        packed.moe_plan(np.zeros((0, 2), dtype=np.int64), 5)
    for bad in (0, 4097, -1, 2.0, True):
        with pytest.raises(hb.MtqError, match="count must be an int in 1 .. 4096"):
            packed.moe_plan(ids, bad)
    with pytest.raises(hb.MtqError, match="backend must be"):
        packed.moe_plan(ids, 5, backend="cuda")
    assert packed.moe_plan(np.zeros((3, 64), dtype=np.int32), 4096).count == 4096        # the limits themselves pass
    plan = packed.moe_plan(ids, 5)
    x = np.zeros((7, 8), dtype=np.float32)
    for bad in (x[:6], x.reshape(-1), np.zeros((8, 8), dtype=np.float32)):
        with pytest.raises(hb.MtqError, match=r"x must be \(7, k\)"):
            packed.moe_dispatch(bad, plan)
    w, ys = np.zeros((7, 2), dtype=np.float32), np.zeros((14, 8), dtype=np.float32)
    for bad in (w[:, :1], w[:6], w.reshape(-1), np.zeros((7, 3), dtype=np.float32)):
        with pytest.raises(hb.MtqError, match=r"topk_weights must be \(7, 2\)"):
            packed.moe_combine(ys, bad, plan)
    with pytest.raises(hb.MtqError, match="topk_weights must be float32"):
        packed.moe_combine(ys, w.astype(np.float64), plan)
    for bad in (ys[:13], ys.reshape(-1), ys[:0]):
        with pytest.raises(hb.MtqError, match=r"ys must be \(14, n\)"):
            packed.moe_combine(bad, w, plan)
    assert packed.moe_combine(np.zeros((20, 8), dtype=np.float32), w, plan).shape == (7, 8)      # more rows are allowed
    for bad in (np.zeros((7, 9), dtype=np.float32), np.zeros((6, 8), dtype=np.float32), np.zeros((8,), dtype=np.float32)):
        with pytest.raises(hb.MtqError, match=r"base must be \(7, 8\)"):
            packed.moe_combine(ys, w, plan, base=bad)
    for bad in ("float16", "float64", None, torch.float32):
        with pytest.raises(hb.MtqError, match="out_dtype must be"):
            packed.moe_combine(ys, w, plan, out_dtype=bad)


# ----------------------------------------------------------------------------- the layer

COUNT, K_IN, HIDDEN, K_OUT = 5, 128, 96, 64


def _experts():
    wg = np.stack([gen("heavy_f32", 30 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wu = np.stack([gen("heavy_f32", 40 + i, (HIDDEN, K_IN)) for i in range(COUNT)])
    wd = np.stack([gen("heavy_f32", 50 + i, (K_OUT, HIDDEN)) for i in range(COUNT)])
    return (packed.pack_batch(wg, np.stack([random_map((HIDDEN, K_IN), 33 + i) for i in range(COUNT)])),
            packed.pack_batch(wu, np.stack([random_map((HIDDEN, K_IN), 43 + i) for i in range(COUNT)])),
            packed.pack_batch(wd, np.stack([random_map((K_OUT, HIDDEN), 53 + i) for i in range(COUNT)])))


def test_packed_moe_on_emulation_is_sort_experts_combine():
    gates, ups, downs = _experts()
    T, K = 11, 2
    rng = np.random.default_rng(9)
    ids = rng.choice(np.array([0, 2, 4, -1, COUNT], dtype=np.int64), size=(T, K))         # experts 1 and 3 empty, some slots dropped
    ids[0] = [4, -1]
    w = (rng.random((T, K)) + 0.25).astype(np.float32)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", 4, (T, K_IN)) * 50)).to(torch.bfloat16)
    base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))).to(torch.bfloat16)
    group_rows, row_of, src = _loop_plan(ids, COUNT)
    R = int(group_rows[-1])
    assert 0 < R < T * K
    for expert_dtype in ("float32", "bfloat16"):
        mlp = packed.PackedExpertsMLP(gates, ups, downs, out_dtype=expert_dtype, backend="emulation")
        ys = mlp(x[torch.from_numpy(src[:R].astype(np.int64) // K)], [int(v) for v in group_rows]).float().numpy()
        for b in (None, base):
            acc = np.zeros((T, K_OUT), dtype=np.float32) if b is None else b.float().numpy().copy()
            for t in range(T):
                for j in range(K):
                    r = int(row_of[t * K + j])
                    if r >= 0:
                        acc[t] = acc[t] + np.float32(w[t, j]) * ys[r]
            for out_dtype in ("bfloat16", "float32"):
                moe = packed.PackedMoE(gates, ups, downs, out_dtype=out_dtype, expert_dtype=expert_dtype, backend="emulation")
                assert moe.backend == "emulation" and moe._plan_workspace is None
                y = moe(x, torch.from_numpy(ids), torch.from_numpy(w), base=b)
                want = torch.from_numpy(acc) if out_dtype == "float32" else torch.from_numpy(acc).to(torch.bfloat16)
                assert y.dtype == want.dtype and tuple(y.shape) == (T, K_OUT)
                words = torch.int32 if out_dtype == "float32" else torch.int16
                assert torch.equal(y.view(words), want.view(words)), (expert_dtype, out_dtype, b is None)
    moe = packed.PackedMoE(gates, ups, downs, decode_max_rows=8)
    assert moe.backend == "emulation" and moe.experts.decode_max_rows == 8 and moe.out_dtype == "bfloat16" and moe.expert_dtype == "float32"
    y3 = moe(x[:10].reshape(2, 5, K_IN), torch.from_numpy(ids[:10]).reshape(2, 5, K), torch.from_numpy(w[:10]).reshape(2, 5, K))
    assert tuple(y3.shape) == (2, 5, K_OUT)
    assert torch.equal(y3.reshape(10, K_OUT).view(torch.int16), moe(x[:10], torch.from_numpy(ids[:10]), torch.from_numpy(w[:10])).view(torch.int16))
    assert tuple(moe(x[:0], torch.from_numpy(ids[:0]), torch.from_numpy(w[:0])).shape) == (0, K_OUT)
    every_dropped = moe(x, torch.full((T, K), -1, dtype=torch.int64), torch.from_numpy(w), base=base)      # R = 0: the base comes back
    assert torch.equal(every_dropped.view(torch.int16), base.view(torch.int16))
    with pytest.raises(hb.MtqError, match=r"x must be \(\.\.\., 128\)"):
        moe(x[:, :64], torch.from_numpy(ids), torch.from_numpy(w))
    with pytest.raises(hb.MtqError, match="topk_ids must be"):
        moe(x, torch.from_numpy(ids[:5]), torch.from_numpy(w[:5]))
    with pytest.raises(hb.MtqError, match="topk_weights must be"):
        moe(x, torch.from_numpy(ids), torch.from_numpy(w[:, :1]))
    with pytest.raises(hb.MtqError, match="base must be"):
        moe(x, torch.from_numpy(ids), torch.from_numpy(w), base=base[:, :32])
    for kw in ({"out_dtype": "float16"}, {"expert_dtype": "float64"}, {"max_tokens": 0}, {"decode_max_rows": -1}, {"act": "gelu"}):
        with pytest.raises(hb.MtqError):
            packed.PackedMoE(gates, ups, downs, **kw)


def _emulated_layer_is_the_loops(moe_of, gates, ups, downs, T, K, ids, seed):
    """PackedMoE on the emulation against _loop_plan, PackedExpertsMLP(backend="emulation") on the sorted rows and _loop_combine."""
    rng = np.random.default_rng(seed)
    w = (rng.random((T, K)) + 0.25).astype(np.float32)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", seed, (T, K_IN)) * 50)).to(torch.bfloat16)
    base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))).to(torch.bfloat16)
    group_rows, row_of, src = _loop_plan(ids, COUNT)
    R = int(group_rows[-1])
    assert 0 < R <= T * K
    for expert_dtype in ("float32", "bfloat16"):
        mlp = packed.PackedExpertsMLP(gates, ups, downs, out_dtype=expert_dtype, backend="emulation")
        ys = np.zeros((T * K, K_OUT), dtype=np.float32)
        ys[:R] = mlp(x[torch.from_numpy(src[:R].astype(np.int64) // K)], [int(v) for v in group_rows]).float().numpy()
        for b in (None, base):
            acc = _loop_combine(row_of, w, ys, None if b is None else b.float().numpy(), T, K)
            for out_dtype in ("bfloat16", "float32"):
                y = moe_of(out_dtype, expert_dtype)(x, torch.from_numpy(ids), torch.from_numpy(w), base=b)
                want = torch.from_numpy(acc) if out_dtype == "float32" else torch.from_numpy(acc).to(torch.bfloat16)
                words = torch.int32 if out_dtype == "float32" else torch.int16
                assert y.dtype == want.dtype and torch.equal(y.view(words), want.view(words)), (T, K, expert_dtype, out_dtype, b is None)


def test_packed_moe_on_emulation_at_the_gpu_files_layer_cases():
    """T = 130, K = 8 (S = 1040, two batches of slots, every token names an expert more than once), uniform and with dropped slots and
    empty experts; then T = 3, K = 8 on the same modules; T = 4, K = 9."""
    gates, ups, downs = _experts()
    modules = {}

    def moe_of(out_dtype, expert_dtype):                  # one module per pair of types for all calls: the small call follows the large one
        if (out_dtype, expert_dtype) not in modules:
            modules[out_dtype, expert_dtype] = packed.PackedMoE(gates, ups, downs, out_dtype=out_dtype, expert_dtype=expert_dtype,
                                                                backend="emulation", max_tokens=1)
        return modules[out_dtype, expert_dtype]

    rng = np.random.default_rng(130)
    for T, K in ((130, 8), (3, 8), (4, 9)):
        assert K > 4 and (T != 130 or T * K > hb.MOE_RUN) and (K != 9 or K > packed.MOE_PLAN_TOPK)
        uniform = rng.integers(0, COUNT, size=(T, K)).astype(np.int64)
        sparse = rng.choice(np.array([0, 2, 4, -1, COUNT, COUNT + 3], dtype=np.int64), size=(T, K))
        sparse[0, :5] = [-1, COUNT, -1, COUNT + 3, 4]     # a token whose first batch of four slots is all dropped
        for seed, ids in enumerate((uniform, sparse)):
            _emulated_layer_is_the_loops(moe_of, gates, ups, downs, T, K, ids, 10 * T + seed)
