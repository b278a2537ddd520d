"""CPU-only: the grouped skinny GLU and the MoE decode entries with a wave per 32-row chunk (include/mtq_glu_chunked.h; kernel= on
packed.glu_grouped_skinny, glu_matmul_grouped_skinny, moe_glu and moe_down_combine; decode_grouped_kernel= on the expert MLPs and
PackedMoE) as far as they go without a device.

  symbols     the twelve names are declared in mtq_glu_chunked.h, which mtq.h includes, in the letters of hip_backend's table and of
              their walking parents, and bound; a library without them loads;
  sizes       each size function is its parent's answer plus the plan region, (count + 1) * 4 rounded up to 16;
  refusals    every rung of each entry's ladder comes back with its walking parent's code and words before a device is looked for (both
              are called with the same host addresses, which no check may dereference); the workspace rungs at every split;
  emulation   kernel= and decode_grouped_kernel= give the "walk" value under every name, on the routings of tests/moe_cases.py;
  arguments   unknown names, a name without decode_max_rows, and "chunks" on a library without the symbols: an MtqError that names
              them before any device work, with the walking binding never called."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_cases
from tests.glu_chunked_cases import COMBINE, ENTRIES, GATHER, GLU, NEW, PARENT, SIZES, plan_bytes
from tests.inputs import gen, to_bf16_valued
from tests.moe_fused_cases import COUNT, HIDDEN, K_IN, K_OUT, STORED, _weights, layer_experts, pack_experts
from tests.test_capi_host import _load, _OnDevice, _StubLibrary
from tests.test_packed_moe_fused_host import _prototypes

INCLUDE = Path(__file__).resolve().parents[1] / "include"
INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -3
BAD_SIZE = 2 ** 64 - 1
KERNELS = ("walk", "chunks", "auto")


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def test_the_entries_are_declared_optional_and_bound():
    assert packed.GLU_SKINNY_GROUPED_KERNELS == KERNELS and packed.GLU_SKINNY_GROUPED_AUTO_KERNEL in ("walk", "chunks")
    text = (INCLUDE / "mtq_glu_chunked.h").read_text(encoding="utf-8")
    lines = (INCLUDE / "mtq.h").read_text(encoding="utf-8").splitlines()
    assert lines.index('#include "mtq_glu_chunked.h"') == lines.index('#include "mtq_moe_decode.h"') + 1      # at the end, next to it
    want = _prototypes(text)
    assert len(NEW) == 12 and set(want) == set(NEW) == set(hb.GLU_CHUNKED_SIGNATURES) == set(hb.GLU_CHUNKED_EXPORTS)
    assert not set(NEW) & (set(hb.SIGNATURES) | set(hb.MOE_DECODE_SIGNATURES))      # a table of its own
    L = hb.lib()
    parents = {**hb.SIGNATURES, **hb.MOE_DECODE_SIGNATURES}
    for name in NEW:
        result, params, optional = hb.GLU_CHUNKED_SIGNATURES[name]
        assert optional is True and (result, params) == want[name], (name, params, want[name])
        assert (result, params) == parents[PARENT[name]][:2], name      # the parent's parameters in the parent's order
        fn = getattr(L, name)
        assert fn.restype is hb._CTYPE[result] and list(fn.argtypes) == [hb._CTYPE[c] for c in params], name
    assert "optional" in text and "bit for bit" in text
    for kn in (False, True):
        assert hb.PACKED_GLU_SKINNY_GROUPED_CHUNKED[kn] == (GLU[kn], GLU[kn] + "_workspace_bytes")
        assert hb.MOE_GATHER_CHUNKED[kn] == (GATHER[kn], GATHER[kn] + "_workspace_bytes")
        assert hb.MOE_DOWN_COMBINE_CHUNKED[kn] == (COMBINE[kn], COMBINE[kn] + "_workspace_bytes")
        assert hb.moe_decode_chunked_bound(kn) is True
    assert hb.glu_grouped_chunked_bound(False) is True and hb.glu_grouped_chunked_bound(True) is True
    assert hb.lib().mtq_version() == hb.MTQ_VERSION == 143
    # what does not change
    assert packed.MOE_DECODE_ROUTES == ("staged", "fused") and packed.GLU_GROUPED_KERNELS == ("fused", "unfused")
    assert packed.GROUPED_KERNELS == packed.MATMUL_GROUPED_KERNELS == ("walk", "chunks", "auto")


SHAPES = ((1, 64, 96), (6, 64, 96), (70, 300, 128), (200, 72, 300), (256, 2048, 7168), (2048, 4096, 14336), (33, 72, 4096))


def test_each_size_function_is_its_parents_plus_the_plan_region():
    assert [plan_bytes(c) for c in (1, 2, 3, 4, 5, 300)] == [16, 16, 16, 32, 32, 1216]
    for count in (1, 5, 300):
        for T, n, k in SHAPES:
            tiles_w = -(-k // 32)
            for split in (0, 1, 2, 3, tiles_w + 3):
                for name in SIZES:
                    got, parent = int(hb._entry(name)(T, count, n, k, split)), int(hb._entry(PARENT[name])(T, count, n, k, split))
                    assert parent != BAD_SIZE and got - parent == plan_bytes(count) and got % 16 == 0, (name, T, count, n, k, split)
                for kn in (False, True):
                    assert hb.moe_glu_gather_workspace_bytes(T, count, n, k, split, kn=kn, kernel="chunks") == \
                        hb.moe_glu_gather_workspace_bytes(T, count, n, k, split, kn=kn) + plan_bytes(count)
                    assert hb.moe_down_combine_workspace_bytes(T, count, n, k, split, kn=kn, kernel="chunks") == \
                        hb.moe_down_combine_workspace_bytes(T, count, n, k, split, kn=kn, kernel="walk") + plan_bytes(count)
                assert hb.glu_grouped_chunked_workspace_bytes(T, count, n, k, split) == \
                    hb.glu_grouped_chunked_workspace_bytes(T, count, n, k, split, kn=True) == \
                    hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, split) + plan_bytes(count)
    for bad in ((0, 5, 64, 96, 0), (-1, 5, 64, 96, 0), (2 ** 31, 1, 8, 32, 0), (6, 0, 64, 96, 0), (6, -3, 64, 96, 0), (6, 5, 0, 96, 0),
                (6, 5, 64, 0, 0), (6, 5, 64, 96, -1), (6, 5, 2 ** 30 + 1, 96, 0)):
        for name in SIZES:
            assert hb._entry(name)(*bad) == BAD_SIZE == hb._entry(PARENT[name])(*bad), (name, bad)
        with pytest.raises(hb.MtqError):
            hb.glu_grouped_chunked_workspace_bytes(*bad)
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        hb.moe_glu_gather_workspace_bytes(6, 5, 64, 96, kernel="auto")      # hip_backend takes resolved names


def _ladder(child, parent, call, rungs, plan):
    """Every rung on both entries: the same code and the same words, the parent's workspace shifted by the plan region."""
    for rc, match, kw in rungs:
        got = call(child, **kw)
        got_words = _last()
        want = call(parent, **kw)
        want_words = _last()
        assert got == want == rc, (kw, got, want)
        assert match in got_words and got_words == want_words, (kw, got_words, want_words)
    return plan


@pytest.mark.parametrize("gather", (False, True))
@pytest.mark.parametrize("kn", (False, True))
def test_the_glu_entries_refuse_what_their_parents_refuse_before_a_device(kn, gather):
    name = (GATHER if gather else GLU)[kn]
    child, parent = hb._entry(name), hb._entry(PARENT[name])
    _buf, p = _aligned()
    T, K, count, n, k = 7, 2, 5, 96, 128
    S, tiles = T * K, 3 * 4
    stream_bytes = count * tiles * 4096                   # above any format's; the arena is never dereferenced

    def call(fn, x=p, T=T, K=K, k=k, ldx=k, src=p, rows=p, gate=p, gate_bytes=stream_bytes, gm=p, go=p, gb=p, up=p, up_bytes=stream_bytes, um=p,
             uo=p, ub=p, count=count, n=n, bg=None, bu=None, ldb=0, act=0, y=p, out=hb.DTYPE_BF16, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        head = (x, T, K, k, ldx, src) if gather else (x, T * K, k, ldx)
        return fn(*head, rows, gate, gate_bytes, gm, go, gb, up, up_bytes, um, uo, ub, count, n, bg, bu, ldb, act, y, out, ldy, split, ws, ws_bytes,
                  None)

    rungs = [(INVALID, "null argument", {a: None}) for a in ("x", "rows", "gate", "gm", "go", "gb", "up", "um", "uo", "ub", "y")]
    rungs += [(INVALID, "out_dtype", dict(out=7)), (INVALID, "count must be positive", dict(count=0)),
              (INVALID, "split must not be negative", dict(split=-1)), (INVALID, "rows and cols must be positive", dict(n=0, ldy=1)),
              (INVALID, "rows and cols must be positive", dict(k=0)), (INVALID, "matrix too large", dict(k=2 ** 30 + 1, ldx=2 ** 31)),
              (INVALID, "ldx < k", dict(ldx=k - 1)), (INVALID, "ldy < n", dict(ldy=n - 1)), (INVALID, "ldb < n", dict(bg=p, ldb=n - 1)),
              (INVALID, "ldb < n", dict(bu=p, ldb=n - 1)), (INVALID, "packed", dict(gate=p + 8)), (INVALID, "packed", dict(up=p + 8)),
              (INVALID, "packed", dict(gate_bytes=64)), (INVALID, "packed", dict(up_bytes=64)), (UNSUPPORTED, "act", dict(act=9)),
              (UNSUPPORTED, "act", dict(act=-1)), (INVALID, "aligned", dict(ws=p + 8))]
    if gather:
        rungs += [(INVALID, "null argument", dict(src=None)), (INVALID, "tokens must be positive", dict(T=0)), (INVALID, "topk must be", dict(K=0)),
                  (INVALID, "topk must be", dict(K=65)), (INVALID, "below 2^31", dict(T=2 ** 30)), (INVALID, "matrix too large", dict(ldx=2 ** 40 + 8)),
                  (INVALID, "not aligned to its type", dict(x=p + 1)), (INVALID, "not aligned to its type", dict(src=p + 2))]
    else:
        rungs += [(INVALID, "total_rows must be positive", dict(T=0)), (INVALID, "does not fit the 32-bit", dict(T=2 ** 30, K=2))]
    # the order of the rungs: with two things wrong, both entries name the same one
    rungs += [(INVALID, "out_dtype", dict(out=7, count=0)), (INVALID, "count must be positive", dict(count=0, ldx=k - 1)),
              (INVALID, "ldx < k", dict(ldx=k - 1, act=9)), (UNSUPPORTED, "act", dict(act=9, ws=None))]
    _ladder(child, parent, call, rungs, plan_bytes(count))
    # the workspace, at every split: null, misaligned, short by one byte - the parent's words with the chunked entry's own bytes
    for split in (0, 1, 2, 3, 4 + 3):
        need, below = int(hb._entry(name + "_workspace_bytes")(S, count, n, k, split)), int(hb._entry(PARENT[name] + "_workspace_bytes")(S, count, n, k, split))
        assert need == below + plan_bytes(count) == below + 32
        for fn, size in ((child, need), (parent, below)):
            assert call(fn, split=split, ws=None) == INVALID and "workspace is null: the partial sums of both projections" in _last()
            assert call(fn, split=split, ws=p + 4) == INVALID and "aligned" in _last()
            assert call(fn, split=split, ws_bytes=size - 1) == INVALID
            assert f"workspace_bytes {size - 1} is smaller than the {size} bytes this split needs" in _last()
        assert call(child, split=split, ws_bytes=below) == INVALID      # the parent's size is not enough
        if not torch.cuda.is_available():                 # everything in order: only the device is missing
            assert call(child, split=split, ws_bytes=need) == NO_DEVICE == call(parent, split=split, ws_bytes=below)
    if not torch.cuda.is_available():
        assert call(child, x=p + 2, ldx=k + 1, bg=p, bu=p, ldb=n, out=hb.DTYPE_F32) == NO_DEVICE


@pytest.mark.parametrize("kn", (False, True))
def test_the_combine_entry_refuses_what_its_parent_refuses_before_a_device(kn):
    name = COMBINE[kn]
    child, parent = hb._entry(name), hb._entry(PARENT[name])
    _buf, p = _aligned()
    T, K, count, n, k = 7, 2, 5, 64, 96
    S, tiles = T * K, 2 * 3
    stream_bytes = count * tiles * 4096

    def call(fn, x=p, k=k, ldx=k, rows=p, packed_=p, nbytes=stream_bytes, maps=p, offs=p, bases=p, count=count, n=n, expert=hb.DTYPE_F32, row_of=p,
             w=p, ldw=K, base=None, base_dtype=0, ldbase=0, T=T, K=K, y=p, out=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        return fn(x, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, expert, row_of, w, ldw, base, base_dtype, ldbase, T, K, y, out,
                  ldy, split, ws, ws_bytes, None)

    rungs = [(INVALID, "null argument", {a: None}) for a in ("x", "rows", "packed_", "maps", "offs", "bases", "row_of", "w", "y")]
    rungs += [(INVALID, "out_dtype", dict(out=2)), (INVALID, "expert_dtype", dict(expert=2)), (INVALID, "expert_dtype", dict(expert=-1)),
              (INVALID, "base_dtype", dict(base=p, base_dtype=5, ldbase=n)), (INVALID, "tokens must be positive", dict(T=0)),
              (INVALID, "topk must be", dict(K=0, ldw=1)), (INVALID, "topk must be", dict(K=65, ldw=65)), (INVALID, "below 2^31", dict(T=2 ** 30)),
              (INVALID, "count must be positive", dict(count=0)), (INVALID, "split must not be negative", dict(split=-1)),
              (INVALID, "rows and cols must be positive", dict(n=0, ldy=1)), (INVALID, "matrix too large", dict(n=2 ** 30 + 1, ldy=2 ** 31)),
              (INVALID, "ldx < k", dict(ldx=k - 1)), (INVALID, "ldy < n", dict(ldy=n - 1)), (INVALID, "packed", dict(packed_=p + 8)),
              (INVALID, "packed", dict(nbytes=64)), (INVALID, "ldw < topk", dict(ldw=K - 1)), (INVALID, "ldbase < n", dict(base=p, ldbase=n - 1)),
              (INVALID, "matrix too large", dict(ldw=2 ** 31 + 1)), (INVALID, "not aligned to its type", dict(y=p + 2)),
              (INVALID, "not aligned to its type", dict(row_of=p + 2)), (INVALID, "not aligned to its type", dict(w=p + 1)),
              (INVALID, "not aligned to its type", dict(base=p + 2, base_dtype=hb.DTYPE_F32, ldbase=n)), (INVALID, "aligned", dict(ws=p + 8)),
              (INVALID, "null argument", dict(w=None, out=2)), (INVALID, "out_dtype", dict(out=2, expert=2)),
              (INVALID, "expert_dtype", dict(expert=2, T=0)), (INVALID, "ldx < k", dict(ldx=k - 1, ldw=K - 1)),
              (INVALID, "ldw < topk", dict(ldw=K - 1, ws=None))]
    _ladder(child, parent, call, rungs, plan_bytes(count))
    for split in (0, 1, 2, 3, 3 + 3):
        need, below = int(hb._entry(name + "_workspace_bytes")(S, count, n, k, split)), int(hb._entry(PARENT[name] + "_workspace_bytes")(S, count, n, k, split))
        assert need == below + 32 and below == min(max(split, 1), 3) * S * n * 4
        for fn, size in ((child, need), (parent, below)):
            assert call(fn, split=split, ws=None) == INVALID and "workspace is null: the experts' partial sums need one at every split" in _last()
            assert call(fn, split=split, ws=p + 4) == INVALID and "aligned" in _last()
            assert call(fn, split=split, ws_bytes=size - 1) == INVALID
            assert f"workspace_bytes {size - 1} is smaller than the {size} bytes this split needs" in _last()
        assert call(child, split=split, ws_bytes=below) == INVALID
        if not torch.cuda.is_available():
            assert call(child, split=split, ws_bytes=need) == NO_DEVICE == call(parent, split=split, ws_bytes=below)


# ----------------------------------------------------------------------------- the emulation: one value under every name

ROUTINGS = tuple(r for r in moe_cases.ROUTINGS if r[2] <= 300 and r[0] * r[1] <= 2048)
KINDS = tuple(kind for kind in moe_cases.KINDS if kind != "high_word")
SMALL = 32


def _words(t):
    t = torch.as_tensor(t)
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


_small = {}


def _small_experts(count, stored):
    if (count, stored) not in _small:
        _small[count, stored] = tuple(packed.as_batch(pack_experts(_weights(count, SMALL, SMALL, seed), seed + 3, stored)) for seed in (30, 40, 50))
    return _small[count, stored]


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("T,K,count", ROUTINGS)
def test_the_emulation_gives_the_walk_value_under_every_kernel_name(T, K, count, stored):
    gate, up, down = _small_experts(count, stored)
    glu = packed.glu_grouped_skinny if stored == "rows" else packed.glu_matmul_grouped_skinny
    rng = np.random.default_rng(T + K)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", T, (T, SMALL)) * 50)).to(torch.bfloat16)
    w = (rng.random((T, K)) + 0.25).astype(np.float32)
    for kind in KINDS[:: 1 if T * K <= 256 else 3]:
        ids = moe_cases._routing(T, K, count, kind, np.int64)
        plan = packed.moe_plan(ids, count, backend="emulation")
        R = int(plan.group_rows[-1])
        xs = packed.moe_dispatch(x, plan)[:R]
        want_glu = glu(xs, plan.group_rows, gate, up, out_dtype="bfloat16", backend="emulation")
        want_h = packed.moe_glu(x, plan, gate, up, stored=stored, backend="emulation")
        want_y = packed.moe_down_combine(want_h, w, plan, down, stored=stored)
        for kernel in KERNELS:
            got = glu(xs, plan.group_rows, gate, up, out_dtype="bfloat16", backend="emulation", kernel=kernel)
            assert torch.equal(_words(got), _words(want_glu)), (kind, kernel)
            assert torch.equal(_words(packed.moe_glu(x, plan, gate, up, stored=stored, backend="emulation", kernel=kernel)), _words(want_h)), (kind, kernel)
            assert torch.equal(_words(packed.moe_down_combine(want_h, w, plan, down, stored=stored, kernel=kernel)), _words(want_y)), (kind, kernel)


@pytest.mark.parametrize("stored", STORED)
def test_the_modules_give_the_default_value_under_every_name_on_the_emulation(stored):
    gates, ups, downs = layer_experts(stored)
    mlp = packed.PackedExpertsMLP if stored == "rows" else packed.PackedExpertsMatmulMLP
    rng = np.random.default_rng(9)
    for T, K in ((7, 2), (64, 8)):
        S = T * K
        x = torch.from_numpy(to_bf16_valued(gen("normal_f32", T, (T, K_IN)) * 50)).to(torch.bfloat16)
        w = torch.from_numpy((rng.random((T, K)) + 0.25).astype(np.float32))
        for kind in ("uniform", "one", "dropped", "none_live"):
            ids = torch.from_numpy(moe_cases._routing(T, K, COUNT, kind, np.int64))
            plan = packed.moe_plan(ids, COUNT, backend="emulation")
            R = int(plan.group_rows[-1])
            xs = packed.moe_dispatch(x, plan)[:R]
            base_mlp = mlp(gates, ups, downs, backend="emulation", decode_max_rows=S)
            assert base_mlp.decode_grouped_kernel == "walk"
            for route in packed.MOE_DECODE_ROUTES:
                kw = dict(backend="emulation", decode_max_rows=S, stored=stored, decode_route=route)
                want = packed.PackedMoE(gates, ups, downs, **kw)(x, ids, w)
                for kernel in KERNELS:
                    moe = packed.PackedMoE(gates, ups, downs, decode_grouped_kernel=kernel, **kw)
                    assert moe.decode_grouped_kernel == moe.experts.decode_grouped_kernel == kernel and moe._fused_workspace is None
                    assert torch.equal(_words(moe(x, ids, w)), _words(want)), (T, K, kind, route, kernel)
            for kernel in KERNELS:
                got = mlp(gates, ups, downs, backend="emulation", decode_max_rows=S, decode_grouped_kernel=kernel)(xs, plan.group_rows)
                assert torch.equal(_words(got), _words(base_mlp(xs, plan.group_rows))), (T, K, kind, kernel)


# ----------------------------------------------------------------------------- arguments

def test_unknown_names_and_names_without_the_decode_route_are_refused():
    gates, ups, downs = layer_experts("rows")
    gate, up, down = (packed.as_batch(b) for b in (gates, ups, downs))
    ids = moe_cases._routing(7, 2, COUNT, "uniform", np.int64)
    plan = packed.moe_plan(ids, COUNT, backend="emulation")
    x, h = torch.zeros((7, K_IN), dtype=torch.bfloat16), torch.zeros((14, HIDDEN), dtype=torch.bfloat16)
    w = np.ones((7, 2), dtype=np.float32)
    for bad in ("chunk", "wide", None, "skinny"):
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.glu_grouped_skinny(x, [0, 7, 7, 7, 7, 7], gate, up, kernel=bad)
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.glu_matmul_grouped_skinny(x, [0, 7, 7, 7, 7, 7], *(packed.as_batch(b) for b in layer_experts("transpose")[:2]), kernel=bad)
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.moe_glu(x, plan, gate, up, kernel=bad)
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.moe_down_combine(h, w, plan, down, kernel=bad)
        for cls in (packed.PackedExpertsMLP, packed.PackedMoE):
            with pytest.raises(hb.MtqError, match="decode_grouped_kernel must be one of"):
                cls(gates, ups, downs, decode_max_rows=8, decode_grouped_kernel=bad)
    with pytest.raises(hb.MtqError, match="decode_grouped_kernel must be one of"):
        packed.PackedExpertsMatmulMLP(*layer_experts("transpose"), decode_max_rows=8, decode_grouped_kernel="fused")
    for kernel in ("chunks", "auto"):
        for cls in (packed.PackedExpertsMLP, packed.PackedMoE):
            with pytest.raises(hb.MtqError, match="needs decode_max_rows"):
                cls(gates, ups, downs, decode_grouped_kernel=kernel)
    assert packed.PackedMoE(gates, ups, downs).decode_grouped_kernel == "walk"      # the default: nothing changes


def _raiser(name):
    def raises(*args, **kwargs):
        raise AssertionError(f"{name} was called in place of the kernel that was asked for")
    return raises


@pytest.mark.parametrize("stored", STORED)
def test_chunks_without_the_symbols_is_refused_before_device_work_and_nothing_stands_in(monkeypatch, stored):
    kn = stored == "transpose"
    gates, ups, downs = layer_experts(stored)
    glu = packed.glu_matmul_grouped_skinny if kn else packed.glu_grouped_skinny
    walking = ("packed_glu_matmul_skinny_grouped" if kn else "packed_glu_skinny_grouped", "moe_glu_gather", "moe_down_combine",
               "packed_matmul_skinny_grouped" if kn else "packed_linear_skinny_grouped")
    for name in walking:
        monkeypatch.setattr(hb, name, _raiser(name))
    monkeypatch.setattr(hb, "glu_grouped_chunked_bound", lambda kn=False: False)
    monkeypatch.setattr(hb, "moe_decode_chunked_bound", lambda kn=False: False)
    monkeypatch.setattr(packed, "batch_to_device", _raiser("batch_to_device"))      # the first device work of every hip call
    x = torch.zeros((7, K_IN), dtype=torch.bfloat16)
    named = ".*".join(hb.PACKED_GLU_SKINNY_GROUPED_CHUNKED[kn]) + ".*lacks.*rebuild it from this tree"
    with pytest.raises(hb.MtqError, match='kernel="chunks".* needs ' + named):
        glu(x, [0, 7, 7, 7, 7, 7], gates, ups, backend="hip", kernel="chunks")
    dev = _OnDevice(torch.zeros((14,), dtype=torch.int32))
    plan = packed.MoEPlan(dev, dev, dev, 7, 2, COUNT)
    moe_named = ".*".join(hb.MOE_GATHER_CHUNKED[kn] + hb.MOE_DOWN_COMBINE_CHUNKED[kn]) + ".*lacks.*rebuild it from this tree"
    with pytest.raises(hb.MtqError, match="moe_glu needs " + moe_named):
        packed.moe_glu(x, plan, gates, ups, stored=stored, kernel="chunks")
    with pytest.raises(hb.MtqError, match="moe_down_combine needs " + moe_named):
        packed.moe_down_combine(torch.zeros((14, HIDDEN), dtype=torch.bfloat16), np.ones((7, 2), dtype=np.float32), plan, downs, stored=stored,
                                kernel="chunks")
    with pytest.raises(hb.MtqError, match='PackedMoE.*fused.*"chunks".* needs ' + moe_named):
        packed.PackedMoE(gates, ups, downs, decode_route="fused", decode_max_rows=64, backend="hip", stored=stored, decode_grouped_kernel="chunks")
    mlp = packed.PackedExpertsMatmulMLP if kn else packed.PackedExpertsMLP
    with pytest.raises(hb.MtqError, match='decode_grouped_kernel="chunks".* needs ' + named):
        mlp(gates, ups, downs, backend="hip", decode_max_rows=64, decode_grouped_kernel="chunks")
    with pytest.raises(hb.MtqError, match='decode_grouped_kernel="chunks".* needs ' + named):
        packed.PackedMoE(gates, ups, downs, backend="hip", decode_max_rows=64, stored=stored, decode_grouped_kernel="chunks")


def test_a_build_without_the_entries_still_loads(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_skinny_grouped.argtypes is not None and stub.mtq_packed_linear_skinny_grouped_combine.argtypes is not None
    assert hb.has_packed_glu_skinny() and hb.moe_decode_bound(False) and hb.moe_decode_bound(True)
    assert not hb.glu_grouped_chunked_bound(False) and not hb.glu_grouped_chunked_bound(True)
    assert not hb.moe_decode_chunked_bound(False) and not hb.moe_decode_chunked_bound(True)
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    gates, ups, _downs = layer_experts("rows")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_skinny_grouped_chunked.*lacks"):
        packed.glu_grouped_skinny(torch.zeros((7, K_IN), dtype=torch.bfloat16), [0, 7, 7, 7, 7, 7], gates, ups, backend="hip", kernel="chunks")
    half = _StubLibrary(143, missing=GLU[1:] + GATHER[1:] + COMBINE[1:])      # the (k, n) twins alone are missing
    assert _load(monkeypatch, half) is half
    assert hb.glu_grouped_chunked_bound(False) and not hb.glu_grouped_chunked_bound(True)
    assert hb.moe_decode_chunked_bound(False) and not hb.moe_decode_chunked_bound(True)


def test_the_entries_list_is_the_tables():
    assert len(ENTRIES) == 6 and all(re.fullmatch(r"mtq_packed_\w+_chunked(_gather|_combine)?", name) for name in ENTRIES)
    assert set(PARENT.values()) <= set(hb.SIGNATURES) | set(hb.MOE_DECODE_SIGNATURES)
