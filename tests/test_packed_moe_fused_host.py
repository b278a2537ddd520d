"""CPU-only: the MoE decode entries without the staging copies (include/mtq_moe_decode.h; packed.moe_glu, packed.moe_down_combine,
PackedMoE(decode_route="fused")) as far as they go without a device.

  symbols     the eight names are declared in mtq_moe_decode.h, which mtq.h includes, in the letters of hip_backend's table, and bound;
  sizes       the combine entries' formula, max(effective split, 1) * S * n * 4 rounded up to 16 with the effective split of the staged
              entry for the same arguments; the gather entries' function is the grouped skinny GLU's; the twins answer alike;
  refusals    every rung of both entries' ladders comes back MTQ_ERR_INVALID with the parent entry's words before a device is looked
              for (the pointers handed in are host addresses that no check may dereference);
  emulation   moe_glu is moe_dispatch + glu_grouped_skinny and moe_down_combine is linear_grouped + moe_combine, on the routings and
              id patterns of tests/moe_cases.py, for both `stored`; PackedMoE(decode_route="fused") equals decode_route="staged";
  arguments   decode_route's errors, and a library without the symbols is an MtqError that names them."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_cases
from tests.inputs import gen, to_bf16_valued
from tests.moe_fused_cases import COUNT, HIDDEN, K_IN, K_OUT, STORED, _weights, down_split, layer_experts, pack_experts
from tests.test_capi_host import _load, _OnDevice, _StubLibrary

INCLUDE = Path(__file__).resolve().parents[1] / "include"
GATHER = ("mtq_packed_glu_skinny_grouped_gather", "mtq_packed_glu_matmul_skinny_grouped_gather")
COMBINE = ("mtq_packed_linear_skinny_grouped_combine", "mtq_packed_matmul_skinny_grouped_combine")
SIZES = tuple(name + "_workspace_bytes" for name in GATHER + COMBINE)
NEW = GATHER + COMBINE + SIZES
INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -3
BAD_SIZE = 2 ** 64 - 1


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def _prototypes(text):
    """Every prototype of a header → (result class, parameter classes) in hip_backend.SIGNATURES' letters."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    scalar = {"int64_t": "l", "uint32_t": "u", "int": "i", "double": "d", "size_t": "z", "uint64_t": "q"}
    sigs = {}
    for ret, name, params in re.findall(r"([\w\s*]*?)\b(mtq_\w+)\s*\(([^)]*)\)\s*;", text):
        classes = "".join("p" if "*" in p else scalar[" ".join(w for w in p.split()[:-1] if w != "const")] for p in params.split(","))
        sigs[name] = ({"int": "i", "size_t": "z"}[ret.split()[-1]], classes)
    return sigs


def test_the_entries_are_declared_optional_and_bound():
    text = (INCLUDE / "mtq_moe_decode.h").read_text(encoding="utf-8")
    assert re.search(r'^#include "mtq_moe_decode\.h"$', (INCLUDE / "mtq.h").read_text(encoding="utf-8"), flags=re.M)
    want = _prototypes(text)
    assert set(want) == set(NEW) == set(hb.MOE_DECODE_SIGNATURES) == set(hb.MOE_DECODE_EXPORTS)
    L = hb.lib()
    for name in NEW:
        result, params, optional = hb.MOE_DECODE_SIGNATURES[name]
        assert optional is True and (result, params) == want[name], (name, params, want[name])
        fn = getattr(L, name)
        assert fn.restype is hb._CTYPE[result] and list(fn.argtypes) == [hb._CTYPE[c] for c in params], name
    assert "optional" in text
    for kn in (False, True):                              # a twin pair: the same parameters in the same order
        assert hb.MOE_GATHER[kn] == (GATHER[kn], GATHER[kn] + "_workspace_bytes") and hb.moe_decode_bound(kn) is True
        assert hb.MOE_DOWN_COMBINE[kn] == (COMBINE[kn], COMBINE[kn] + "_workspace_bytes")
    assert want[GATHER[0]] == want[GATHER[1]] and want[COMBINE[0]] == want[COMBINE[1]]
    # the gather entry: the staged entry's parameters with (tokens, topk) for total_rows and src in front of group_rows
    staged = hb.SIGNATURES["mtq_packed_glu_skinny_grouped"][1]
    assert want[GATHER[0]][1] == "pll" + staged[2:4] + "p" + staged[4:]
    assert all(want[name] == ("z", "lllli") for name in SIZES)
    assert packed.MOE_DECODE_ROUTES == ("staged", "fused")


SHAPES = ((1, 5, 64, 96), (6, 5, 64, 96), (24, 5, 8, 96), (70, 5, 300, 128), (8, 256, 2048, 7168), (16, 8, 4096, 14336), (256, 8, 4096, 14336),
          (33, 1, 72, 4096), (2 ** 31 - 1, 1, 8, 32))


def test_the_size_functions_give_the_formula_and_never_zero():
    for S, count, n, k in SHAPES:
        for split in (0, 1, 2, 3, 1000):
            eff = down_split(S, count, n, k, split)
            assert eff == min(split, -(-k // 32)) or split == 0
            want = (eff * S * n * 4 + 15) // 16 * 16
            for kn in (False, True):
                assert hb.moe_down_combine_workspace_bytes(S, count, n, k, split, kn=kn) == want > 0, (S, count, n, k, split)
                assert hb.moe_glu_gather_workspace_bytes(S, count, n, k, split, kn=kn) == hb.packed_glu_skinny_grouped_workspace_bytes(S, count, n, k, split)
    assert hb.moe_down_combine_workspace_bytes(1, 1, 1, 1) == 16 and hb.packed_linear_skinny_grouped_workspace_bytes(1, 1, 1, 1) == 0
    assert down_split(8, 256, 2048, 7168, 0) == 1 and down_split(16, 8, 4096, 14336, 0) > 1      # the library's own choice goes both ways
    for bad in ((0, 5, 64, 96, 0), (-1, 5, 64, 96, 0), (2 ** 31, 1, 8, 32, 0), (6, 0, 64, 96, 0), (6, 5, 0, 96, 0), (6, 5, 64, 0, 0),
                (6, 5, 64, 96, -1), (6, 5, 2 ** 30 + 1, 96, 0)):
        for name in SIZES:
            assert hb._entry(name)(*bad) == BAD_SIZE, (name, bad)
        with pytest.raises(hb.MtqError):
            hb.moe_down_combine_workspace_bytes(*bad)
        with pytest.raises(hb.MtqError):
            hb.moe_glu_gather_workspace_bytes(*bad)


@pytest.mark.parametrize("kn", (False, True))
def test_the_gather_entry_refuses_before_a_device(kn):
    fn = hb._entry(GATHER[kn])
    _buf, p = _aligned()
    T, K, count, n, k = 7, 2, 5, 96, 128
    S, tiles = T * K, 3 * 4
    stream_bytes = count * tiles * 4096                   # above any format's; the arena is never dereferenced
    need = hb.moe_glu_gather_workspace_bytes(S, count, n, k, 0, kn=kn)

    def call(x=p, T=T, K=K, k=k, ldx=k, src=p, rows=p, gate=p, gate_bytes=stream_bytes, gm=p, go=p, gb=p, up=p, up_bytes=stream_bytes, um=p, uo=p,
             ub=p, count=count, n=n, bg=None, bu=None, ldb=0, act=0, y=p, out=hb.DTYPE_BF16, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        return fn(x, T, K, k, ldx, src, rows, gate, gate_bytes, gm, go, gb, up, up_bytes, um, uo, ub, count, n, bg, bu, ldb, act, y, out, ldy,
                  split, ws, ws_bytes, None)

    def refused(match, rc=INVALID, **kw):
        assert call(**kw) == rc, kw
        assert match in _last(), _last()

    for name in ("x", "src", "rows", "gate", "gm", "go", "gb", "up", "um", "uo", "ub", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", out=7)
    refused("tokens must be positive", T=0)               # what mtq_moe_plan and mtq_moe_dispatch refuse
    refused("topk must be", K=0)
    refused("topk must be", K=65)
    refused("below 2^31", T=2 ** 30)
    refused("count must be positive", count=0)            # what mtq_packed_glu_skinny_grouped refuses
    refused("split must not be negative", split=-1)
    refused("rows and cols must be positive", n=0, ldy=1)
    refused("rows and cols must be positive", k=0)
    refused("matrix too large", k=2 ** 30 + 1, ldx=2 ** 31)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bg=p, ldb=n - 1)
    refused("packed", gate=p + 8)
    refused("packed", up=p + 8)
    refused("packed", gate_bytes=64)
    refused("matrix too large", ldx=2 ** 40 + 8)
    refused("not aligned to its type", x=p + 1)
    refused("not aligned to its type", src=p + 2)
    refused("act", rc=UNSUPPORTED, act=9)
    refused("workspace is null", ws=None)
    refused("aligned", ws=p + 8)
    refused("smaller than the", ws_bytes=need - 1)
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert call() == NO_DEVICE and call(ws_bytes=need) == NO_DEVICE and call(x=p + 2, ldx=k + 1, bg=p, bu=p, ldb=n) == NO_DEVICE


@pytest.mark.parametrize("kn", (False, True))
def test_the_combine_entry_refuses_before_a_device(kn):
    fn = hb._entry(COMBINE[kn])
    _buf, p = _aligned()
    T, K, count, n, k = 7, 2, 5, 64, 96
    S, tiles = T * K, 2 * 3
    stream_bytes = count * tiles * 4096                   # above any format's; the arena is never dereferenced
    need = hb.moe_down_combine_workspace_bytes(S, count, n, k, 0, kn=kn)
    assert need == S * n * 4

    def call(x=p, k=k, ldx=k, rows=p, packed_=p, nbytes=stream_bytes, maps=p, offs=p, bases=p, count=count, n=n, expert=hb.DTYPE_F32, row_of=p,
             w=p, ldw=K, base=None, base_dtype=0, ldbase=0, T=T, K=K, y=p, out=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        return fn(x, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, expert, row_of, w, ldw, base, base_dtype, ldbase, T, K, y, out,
                  ldy, split, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "rows", "packed_", "maps", "offs", "bases", "row_of", "w", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", out=2)
    refused("expert_dtype", expert=2)
    refused("expert_dtype", expert=-1)
    refused("base_dtype", base=p, base_dtype=5, ldbase=n)
    refused("tokens must be positive", T=0)               # what mtq_moe_combine refuses
    refused("topk must be", K=0, ldw=1)
    refused("topk must be", K=65, ldw=65)
    refused("below 2^31", T=2 ** 30)
    refused("count must be positive", count=0)            # what mtq_packed_linear_skinny_grouped refuses
    refused("split must not be negative", split=-1)
    refused("rows and cols must be positive", n=0, ldy=1)
    refused("matrix too large", n=2 ** 30 + 1, ldy=2 ** 31)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("packed", packed_=p + 8)
    refused("packed", nbytes=64)
    refused("ldw < topk", ldw=K - 1)
    refused("ldbase < n", base=p, ldbase=n - 1)
    refused("matrix too large", ldw=2 ** 31 + 1)
    refused("not aligned to its type", y=p + 2)
    refused("not aligned to its type", row_of=p + 2)
    refused("not aligned to its type", w=p + 1)
    refused("not aligned to its type", base=p + 2, base_dtype=hb.DTYPE_F32, ldbase=n)
    refused("workspace is null", ws=None)                 # at an effective split of 1 too: the partial sums go through it at every split
    refused("aligned", ws=p + 8)
    refused("smaller than the", ws_bytes=need - 1)
    refused("smaller than the", split=2, ws_bytes=2 * need - 1)
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(ws_bytes=need) == NO_DEVICE and call(split=2, ws_bytes=2 * need) == NO_DEVICE
        assert call(base=p + 2, base_dtype=hb.DTYPE_BF16, ldbase=n + 1, out=hb.DTYPE_BF16, y=p + 2, ldy=n + 3, expert=hb.DTYPE_BF16) == NO_DEVICE


# ----------------------------------------------------------------------------- the emulation: the stages composed

ROUTINGS = tuple(r for r in moe_cases.ROUTINGS if r[2] <= 300 and r[0] * r[1] <= 2048)
KINDS = tuple(kind for kind in moe_cases.KINDS if kind != "high_word")
SMALL = 32                                                # experts of 32 → 32 → 32: one tile each, so 300 of them stay quick


def _words(t):
    t = torch.as_tensor(t)
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


_small = {}


def _small_experts(count, stored):
    if (count, stored) not in _small:
        _small[count, stored] = tuple(packed.as_batch(pack_experts(_weights(count, SMALL, SMALL, seed), seed + 3, stored)) for seed in (30, 40, 50))
    return _small[count, stored]


def test_the_routings_cover_the_shared_table():
    assert len(ROUTINGS) >= 6 and (7, 2, 5) in ROUTINGS and (300, 6, 300) in ROUTINGS and (256, 8, 256) in ROUTINGS
    assert {"uniform", "one", "twice", "dropped", "none_live", "distinct"} == set(KINDS)


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("T,K,count", ROUTINGS)
def test_the_emulated_stages_are_the_staged_emulation(T, K, count, stored):
    gate, up, down = _small_experts(count, stored)
    o_glu, o_grouped = (packed.glu_grouped_skinny, packed.linear_grouped) if stored == "rows" else (packed.glu_matmul_grouped_skinny, packed.matmul_grouped)
    rng = np.random.default_rng(T + K)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", T, (T, SMALL)) * 50)).to(torch.bfloat16)
    w = (rng.random((T, K)) + 0.25).astype(np.float32)
    base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, SMALL)).astype(np.float32))).to(torch.bfloat16)
    for kind in KINDS:
        ids = moe_cases._routing(T, K, count, kind, np.int64)
        plan = packed.moe_plan(ids, count, backend="emulation")
        moe_cases.check_kind(kind, ids, count, (plan.group_rows, plan.row_of, plan.src))
        R, S = int(plan.group_rows[-1]), T * K
        # the staged emulation, stage by stage as PackedMoE runs it
        xs = packed.moe_dispatch(x, plan)
        h_want = torch.zeros((S, SMALL), dtype=torch.bfloat16)
        if R:
            h_want[:R] = o_glu(xs[:R], plan.group_rows, gate, up, out_dtype="bfloat16", backend="emulation")
        h = packed.moe_glu(x, plan, gate, up, stored=stored, backend="emulation")
        assert h.dtype == torch.bfloat16 and tuple(h.shape) == (S, SMALL) and torch.equal(_words(h), _words(h_want)), (kind, "moe_glu")
        for expert_dtype in ("float32", "bfloat16"):
            ys = torch.zeros((S, SMALL), dtype=torch.float32 if expert_dtype == "float32" else torch.bfloat16)
            if R:
                ys[:R] = torch.as_tensor(o_grouped(h_want[:R], plan.group_rows, down, out_dtype=expert_dtype, backend="emulation"))
            for b in (None, base):
                for out_dtype in ("float32", "bfloat16"):
                    want = packed.moe_combine(ys, w, plan, base=b, out_dtype=out_dtype)
                    got = packed.moe_down_combine(h, w, plan, down, base=b, expert_dtype=expert_dtype, out_dtype=out_dtype, stored=stored)
                    assert torch.equal(_words(got), _words(want)), (kind, expert_dtype, out_dtype, b is None)


@pytest.mark.parametrize("stored", STORED)
def test_fused_on_the_emulation_equals_staged_on_it(stored):
    gates, ups, downs = layer_experts(stored)
    rng = np.random.default_rng(5)
    for T, K, decode_max_rows in ((3, 2, 64), (32, 8, 256), (130, 8, 256), (4, 9, 64)):
        S = T * K
        x = torch.from_numpy(to_bf16_valued(gen("normal_f32", T, (T, K_IN)) * 50)).to(torch.bfloat16)
        w = torch.from_numpy((rng.random((T, K)) + 0.25).astype(np.float32))
        base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))).to(torch.bfloat16)
        uniform = rng.integers(0, COUNT, size=(T, K)).astype(np.int64)
        sparse = rng.choice(np.array([0, 2, 4, -1, COUNT, COUNT + 3], dtype=np.int64), size=(T, K))
        for ids in (uniform, sparse):
            for expert_dtype in ("float32", "bfloat16"):
                for out_dtype in ("bfloat16", "float32"):
                    kw = dict(out_dtype=out_dtype, expert_dtype=expert_dtype, backend="emulation", decode_max_rows=decode_max_rows, stored=stored)
                    staged, fused = packed.PackedMoE(gates, ups, downs, **kw), packed.PackedMoE(gates, ups, downs, decode_route="fused", **kw)
                    assert staged.decode_route == "staged" and fused.decode_route == "fused" and fused._fused_workspace is None
                    assert (S <= decode_max_rows) == (T != 130)           # T = 130 falls to the staged route inside the fused module
                    for b in (None, base):
                        for ids_t in (torch.from_numpy(ids), torch.from_numpy(ids).to(torch.int32)):
                            got, want = fused(x, ids_t, w, base=b), staged(x, ids_t, w, base=b)
                            assert got.dtype == want.dtype and torch.equal(_words(got), _words(want)), (T, K, expert_dtype, out_dtype, b is None)
    lead = fused(x.reshape(2, 2, K_IN), torch.from_numpy(uniform).reshape(2, 2, K), w.reshape(2, 2, K))
    assert tuple(lead.shape) == (2, 2, K_OUT)


def test_every_argument_error():
    gates, ups, downs = layer_experts("rows")
    with pytest.raises(hb.MtqError, match="decode_route must be one of"):
        packed.PackedMoE(gates, ups, downs, decode_route="fast")
    with pytest.raises(hb.MtqError, match="decode_route must be one of"):
        packed.PackedMoE(gates, ups, downs, decode_route=None, decode_max_rows=8)
    with pytest.raises(hb.MtqError, match='"fused" needs decode_max_rows'):
        packed.PackedMoE(gates, ups, downs, decode_route="fused")
    assert packed.PackedMoE(gates, ups, downs).decode_route == "staged"                   # the default: nothing changes
    ids = moe_cases._routing(7, 2, COUNT, "dropped", np.int64)
    plan = packed.moe_plan(ids, COUNT, backend="emulation")
    x, h = torch.zeros((7, K_IN), dtype=torch.bfloat16), torch.zeros((14, HIDDEN), dtype=torch.bfloat16)
    w = np.ones((7, 2), dtype=np.float32)
    gate, up, down = (packed.as_batch(b) for b in (gates, ups, downs))
    for kw, match in (({"stored": "columns"}, "stored must be one of"), ({"act": "gelu"}, "act"), ({"out_dtype": "float16"}, "out_dtype must be"),
                      ({"backend": "cuda"}, "backend must be one of"), ({"backend": "hip"}, "needs a plan made on it")):
        with pytest.raises(hb.MtqError, match=match):
            packed.moe_glu(x, plan, gate, up, **kw)
    with pytest.raises(hb.MtqError, match=r"x must be \(7, 128\)"):
        packed.moe_glu(x[:6], plan, gate, up)
    with pytest.raises(hb.MtqError, match="as many experts of one shape"):
        packed.moe_glu(x, plan, gate, down)
    with pytest.raises(hb.MtqError, match="the plan is for 4 experts, the batches hold 5"):
        packed.moe_glu(x, packed.moe_plan(ids, 4, backend="emulation"), gate, up)
    for kw, match in (({"stored": "columns"}, "stored must be one of"), ({"out_dtype": "float16"}, "out_dtype must be"),
                      ({"expert_dtype": "float64"}, "expert_dtype must be"), ({"backend": "hip"}, "needs a plan made on it"),
                      ({"base": torch.zeros((7, 32))}, "base must be")):
        with pytest.raises(hb.MtqError, match=match):
            packed.moe_down_combine(h, w, plan, down, **kw)
    with pytest.raises(hb.MtqError, match=r"h must be \(14, 96\)"):
        packed.moe_down_combine(h[:13], w, plan, down)
    with pytest.raises(hb.MtqError, match="topk_weights must be"):
        packed.moe_down_combine(h, w[:, :1], plan, down)
    with pytest.raises(hb.MtqError, match="topk_weights must be float32"):
        packed.moe_down_combine(h, w.astype(np.float64), plan, down)


@pytest.mark.parametrize("stored", STORED)
def test_a_build_without_the_entries_still_loads_and_nothing_stands_in(monkeypatch, stored):
    kn = stored == "transpose"
    lacking = hb.MOE_GATHER[kn] + hb.MOE_DOWN_COMBINE[kn]
    stub = _StubLibrary(143, missing=lacking)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_skinny_grouped.argtypes is not None and stub.mtq_moe_combine.argtypes is not None      # every other symbol is bound
    assert hb.has_moe() and hb.has_packed_glu_skinny() and not hb.moe_decode_bound(kn) and hb.moe_decode_bound(not kn)
    for name in lacking:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    named = ".*".join(lacking) + ".*lacks.*rebuild it from this tree"
    gates, ups, downs = layer_experts(stored)
    dev = _OnDevice(torch.zeros((14,), dtype=torch.int32))
    plan = packed.MoEPlan(dev, dev, dev, 7, 2, COUNT)
    with pytest.raises(hb.MtqError, match="moe_glu needs " + named):
        packed.moe_glu(torch.zeros((7, K_IN), dtype=torch.bfloat16), plan, gates, ups, stored=stored)
    with pytest.raises(hb.MtqError, match="moe_down_combine needs " + named):
        packed.moe_down_combine(torch.zeros((14, HIDDEN), dtype=torch.bfloat16), np.ones((7, 2), dtype=np.float32), plan, downs, stored=stored)
    with pytest.raises(hb.MtqError, match="PackedMoE.*fused.*needs " + named):
        packed.PackedMoE(gates, ups, downs, decode_route="fused", decode_max_rows=64, backend="hip", stored=stored)
