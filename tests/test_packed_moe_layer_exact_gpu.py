"""GPU: the packed MLP and MoE layers against the float64 reference of tests/moe_layer_cases.py on every way through the device:
`stored` rows and transpose, each with the wide route (decode_max_rows=None), the staged decode route and the fused decode route, both
decode routes with the "walk" and the "chunks" grouped kernels.  No kernel of this library stands on the want-side.

  exact   integer-grid inputs, act="none": every float32 operation is exact in any order, so the layer must EQUAL float64: float32
          values (zeros of either sign are equal) and the words wherever the reference is not zero.  Every (layer, routing) pair,
          expert_dtype x out_dtype, no base / a bf16 base / a float32 base, int32 and int64 ids.  (130, 8) has S = 1040 above
          decode_max_rows = 256: the wide route inside every decode module, a fused one included.
  silu    heavy-tailed weights, act="silu", the router's weights: within the derived bound, and (asserted on the want-side) gate and up
          exchanged would not be.  forward as well as forward_logits, whose reference takes ids and weights from want_select on the
          scores the router emitted, so the layer check does not hang on the router's last-ulp choices.
  alone   PackedExpertsMLP / PackedExpertsMatmulMLP on plan.group_rows, and the walking skinny entries written out into sentinels (the
          rows of no group keep them); PackedMLP / PackedMatmulMLP with decode_kernel "pair" and "fused" at m = 1, 5, 32, 33.

Each test derives from the shape which route a call met (S against decode_max_rows; the hot expert's chunk count) and asserts it."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_layer_cases as mc
from tests.glu_chunked_cases import chunks
from tests.moe_cases import SENTINEL
from tests.moe_fused_cases import down_split, glu_split
from tests.moe_route_cases import want_select

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ROWS = mc.DECODE_MAX_ROWS
# (name, decode_max_rows, decode_route, decode_grouped_kernel)
ROUTES = (("wide", None, "staged", "walk"), ("staged-walk", ROWS, "staged", "walk"), ("staged-chunks", ROWS, "staged", "chunks"),
          ("fused-walk", ROWS, "fused", "walk"), ("fused-chunks", ROWS, "fused", "chunks"))
ROUTE_IDS = [r[0] for r in ROUTES]
EXPERT_ROUTES = (("wide", None, "walk"), ("walk", ROWS, "walk"), ("chunks", ROWS, "chunks"))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _bits(t) -> np.ndarray:
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)).cpu().numpy()


def _torch_dtype(name):
    return BF16 if name == "bfloat16" else F32


@functools.lru_cache(maxsize=None)
def _batches(layer, tier, stored):
    """The three device batches of a layer, resolved once: every module of a test multiplies with these arenas."""
    return tuple(packed.batch_to_device(packed.as_batch(p)) for p in mc.experts(layer, tier, stored, "hip"))


def _moe(layer, tier, stored, route, expert_dtype, out_dtype, router=None):
    _name, rows, decode_route, kernel = route
    return packed.PackedMoE(*_batches(layer, tier, stored), act="none" if tier == "exact" else "silu", out_dtype=out_dtype, expert_dtype=expert_dtype,
                            decode_max_rows=rows, max_tokens=1, stored=stored, router=router, decode_route=decode_route, decode_grouped_kernel=kernel)


def _met(route, S) -> str:
    """The way a call of S slots takes through a module of this route, from the shape."""
    _name, rows, decode_route, kernel = route
    return "wide" if rows is None or S > rows else f"{decode_route}-{kernel}"


def _equal(got, want32, out_dtype, what):
    assert got.dtype == _torch_dtype(out_dtype) and tuple(got.shape) == want32.shape, what
    g = got.float().cpu().numpy()
    assert np.array_equal(g, want32), (what, np.argwhere(g != want32)[:4])               # values: zeros of either sign are equal
    nz = want32 != 0
    assert np.array_equal(_bits(got)[nz], _bits(torch.from_numpy(np.array(want32)).to(got.dtype))[nz]), (what, "words")


def _within(got, want, bound, out_dtype, what) -> float:
    assert got.dtype == _torch_dtype(out_dtype) and tuple(got.shape) == want.shape, what
    err = np.abs(got.double().cpu().numpy() - want)
    assert np.all(err <= bound), (what, np.argwhere(err > bound)[:4], float((err / bound).max()))
    return float((err / bound).max())


def _sentinels(rows, pitch, dtype):
    return torch.full((rows * pitch * (2 if dtype == BF16 else 4),), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).view(rows, pitch)


# ----------------------------------------------------------------------------- PackedMoE

@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("stored", mc.STORED)
def test_the_layer_equals_the_exact_reference(stored, route):
    met = {}
    for layer, T, K in mc.PAIRS:
        count, S = mc.LAYERS[layer][0], T * K
        x, ids, w, base = mc.exact_inputs(layer, T, K)
        mc.check_routing(ids, count)
        group_rows, _R, _token, _expert = mc.rows_of_plan(ids, count)
        path = _met(route, S)
        assert (path == "wide") == (route[1] is None or (T, K) == (130, 8)) and (path == "wide" or path == route[0])
        assert (T, K) != (32, 8) or (S == ROWS and int(np.diff(chunks(group_rows, S)).max()) >= 3)      # the last decode size; a third chunk
        _count, k_in, hidden, k_out = mc.LAYERS[layer]
        splits = (glu_split(S, count, hidden, k_in, 0), down_split(S, count, k_out, hidden, 0))      # the library's own choice, which the modules take
        assert splits == ((2, 2) if layer == "long" else (1, 1))       # the long layer: slices summed in both decode stages' reduces
        xd, wd, ids64, ids32 = _dev(x, BF16), _dev(w), _dev(ids), _dev(ids.astype(np.int32))
        plan = packed.moe_plan(ids64, count)
        assert plan.slots == S and np.array_equal(plan.group_rows.cpu().numpy(), group_rows)
        for expert_dtype in mc.DTYPES:
            for out_dtype in mc.DTYPES:
                moe = _moe(layer, "exact", stored, route, expert_dtype, out_dtype)
                assert moe.backend == "hip" and (moe._fused_workspace is not None) == (route[2] == "fused")
                for kind in mc.BASES:
                    want = mc.exact_want(layer, stored, T, K, expert_dtype, out_dtype, kind is not None)[0]
                    b = None if kind is None else _dev(base, _torch_dtype(kind))
                    for ids_d in (ids64, ids32):
                        _equal(moe(xd, ids_d, wd, base=b), want, out_dtype, (layer, T, K, expert_dtype, out_dtype, kind, str(ids_d.dtype)))
                        met[path] = met.get(path, 0) + 1
    print(f"exact: stored={stored} module={route[0]}: comparisons per route met: {met}")


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("stored", mc.STORED)
def test_the_silu_layer_is_within_the_derived_bound(stored, route):
    met = {}
    for layer, T, name in mc.SILU_CASES:
        count = mc.LAYERS[layer][0]
        x, logits, bias, base, ids, w = mc.silu_inputs(layer, T, name)
        r = mc.router(layer, name)
        S = T * r.topk
        path = _met(route, S)
        sizes = np.bincount(ids.reshape(-1), minlength=count)
        assert (path == "wide") == (route[1] is None or T == 130) and (T < 37 or sizes.max() > 32)        # from T = 37 on a second chunk
        xd, wd, ids_d = _dev(x, BF16), _dev(w), _dev(ids)
        logits_d, bias_d = _dev(logits), None if bias is None else _dev(bias)
        _pw, _pids, scores = packed.moe_route(logits_d, r.topk, r.score, bias_d, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale,
                                              return_scores=True)
        sel_ids, sel_w = want_select(scores.cpu().numpy(), bias, r.topk, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale)
        worst = [0.0, 0.0]
        for expert_dtype in mc.DTYPES:
            for out_dtype in mc.DTYPES:
                moe = _moe(layer, "silu", stored, route, expert_dtype, out_dtype, router=r)
                for b in (None, base):
                    bd = None if b is None else _dev(b, BF16)
                    what = (layer, T, name, expert_dtype, out_dtype, b is None)
                    mc.check_exchange_is_seen(layer, stored, T, name, ids, w, b, expert_dtype, out_dtype)
                    want, bound = mc.silu_want(layer, stored, T, name, ids, w, b, expert_dtype, out_dtype)
                    worst[0] = max(worst[0], _within(moe(xd, ids_d, wd, base=bd), want, bound, out_dtype, what + ("forward",)))
                    mc.check_exchange_is_seen(layer, stored, T, name, sel_ids, sel_w, b, expert_dtype, out_dtype)
                    want, bound = mc.silu_want(layer, stored, T, name, sel_ids, sel_w, b, expert_dtype, out_dtype)
                    got = moe.forward_logits(xd, logits_d, bias=bias_d, base=bd)
                    worst[1] = max(worst[1], _within(got, want, bound, out_dtype, what + ("forward_logits",)))
                    met[path] = met.get(path, 0) + 2
        print(f"silu: stored={stored} module={route[0]} met={path} {layer} T={T} {name}: max error / bound = {worst[0]:.4f} (forward), "
              f"{worst[1]:.4f} (forward_logits)")
    print(f"silu: stored={stored} module={route[0]}: comparisons per route met: {met}")


# ----------------------------------------------------------------------------- the expert modules alone

@pytest.mark.parametrize("route", EXPERT_ROUTES, ids=[r[0] for r in EXPERT_ROUTES])
@pytest.mark.parametrize("stored", mc.STORED)
def test_the_expert_modules_alone_on_the_plan(stored, route):
    _name, rows, kernel = route
    cls = packed.PackedExpertsMLP if stored == "rows" else packed.PackedExpertsMatmulMLP
    n = 0
    for layer, T, K in mc.PAIRS:
        count, S = mc.LAYERS[layer][0], T * K
        x, ids, _w, _base = mc.exact_inputs(layer, T, K)
        _group_rows, R, token, expert = mc.rows_of_plan(ids, count)
        plan = packed.moe_plan(_dev(ids), count)
        xs = packed.moe_dispatch(_dev(x, BF16), plan)
        d = mc.exact_rows(layer, stored, T, K)[0][token, expert]
        assert 0 < R < S and (rows is None or (S <= rows) == ((T, K) != (130, 8)))
        for out_dtype in mc.DTYPES:
            mlp = cls(*_batches(layer, "exact", stored), act="none", out_dtype=out_dtype, decode_max_rows=rows, decode_grouped_kernel=kernel)
            y = mlp(xs, plan.group_rows)
            assert tuple(y.shape) == (S, mc.LAYERS[layer][3])
            _equal(y[:R], (mc._bf16(d) if out_dtype == "bfloat16" else d).astype(np.float32), out_dtype, (layer, T, K, out_dtype))
            n += 1
    for layer, T, name in mc.SILU_CASES:
        count = mc.LAYERS[layer][0]
        x, _logits, _bias, _base, ids, _w = mc.silu_inputs(layer, T, name)
        _group_rows, R, token, expert = mc.rows_of_plan(ids, count)
        plan = packed.moe_plan(_dev(ids), count)
        xs = packed.moe_dispatch(_dev(x, BF16), plan)
        d, e_d = (a[token, expert] for a in mc.silu_rows(layer, stored, T, name))
        worst = 0.0
        for out_dtype in mc.DTYPES:
            mlp = cls(*_batches(layer, "silu", stored), act="silu", out_dtype=out_dtype, decode_max_rows=rows, decode_grouped_kernel=kernel)
            want, bound = mc._store_bf16(d, e_d) if out_dtype == "bfloat16" else (d, e_d)
            worst = max(worst, _within(mlp(xs, plan.group_rows)[:R], want, bound, out_dtype, (layer, T, name, out_dtype)))
            n += 1
        print(f"experts alone, silu: stored={stored} {route[0]} {layer} T={T} {name}: max error / bound = {worst:.4f}")
    print(f"experts alone: stored={stored} {route[0]}: {n} comparisons")


@pytest.mark.parametrize("stored", mc.STORED)
def test_the_walking_entries_leave_the_rows_of_no_group_alone(stored):
    """The staged decode route written out on the entries that take `out`: the grouped skinny GLU into bf16, the grouped skinny
    product on it, both into sentinels.  The rows of a group equal the exact reference; the rows from R on keep their sentinel."""
    kn = stored == "transpose"
    glu = hb.packed_glu_matmul_skinny_grouped if kn else hb.packed_glu_skinny_grouped
    down = hb.packed_matmul_skinny_grouped if kn else hb.packed_linear_skinny_grouped
    for layer, T, K in (("even", 37, 2), ("ragged", 32, 8), ("long", 37, 2)):
        count, _k_in, hidden, k_out = mc.LAYERS[layer]
        S = T * K
        x, ids, _w, _base = mc.exact_inputs(layer, T, K)
        _group_rows, R, token, expert = mc.rows_of_plan(ids, count)
        assert 0 < R < S
        plan = packed.moe_plan(_dev(ids), count)
        xs = packed.moe_dispatch(_dev(x, BF16), plan)
        arenas = [(b.arena, b.maps_dev, b.offsets_dev, b.bases_dev) for b in _batches(layer, "exact", stored)]
        d = mc.exact_rows(layer, stored, T, K)[0][token, expert]
        for split in (0, 3):                              # the library's choice (2 on the long layer, else 1), and three slices
            assert glu_split(S, count, hidden, _k_in, split) == down_split(S, count, k_out, hidden, split) == (split or (2 if layer == "long" else 1))
            h = _sentinels(S + 2, hidden, BF16)
            glu(xs, plan.group_rows, arenas[0], arenas[1], count, hidden, act="none", out_dtype=BF16, out=h[:S], split=split)
            assert bool((h.view(torch.uint8).view(S + 2, -1)[R:] == SENTINEL).all()), "a row of h of no group was written"
            for out_dtype in mc.DTYPES:
                y = _sentinels(S + 2, k_out + 8, _torch_dtype(out_dtype))
                got = down(h[:S], plan.group_rows, *arenas[2], count, k_out, out_dtype=_torch_dtype(out_dtype), out=y[:S, :k_out], split=split)
                assert got.data_ptr() == y.data_ptr()
                _equal(y[:R, :k_out], (mc._bf16(d) if out_dtype == "bfloat16" else d).astype(np.float32), out_dtype, (layer, T, K, out_dtype, split))
                raw = y.view(torch.uint8).view(S + 2, -1)
                width = k_out * (2 if out_dtype == "bfloat16" else 4)
                assert bool((raw[R:] == SENTINEL).all()) and bool((raw[:, width:] == SENTINEL).all()), "a row of no group, or a byte past a row, was written"


# ----------------------------------------------------------------------------- the dense modules

@pytest.mark.parametrize("decode_kernel", ("pair", "fused"))
@pytest.mark.parametrize("stored", mc.STORED)
def test_the_dense_modules_alone(stored, decode_kernel):
    cls = packed.PackedMLP if stored == "rows" else packed.PackedMatmulMLP
    assert packed.SKINNY_MAX_M == 32 and mc.DENSE_M == (1, 5, 32, 33)                     # the skinny range and the first row past it
    n = 0
    for layer in mc.LAYERS:
        for tier, act in (("exact", "none"), ("silu", "silu")):
            one = mc.dense_experts(layer, tier, stored, "hip")
            worst = 0.0
            for out_dtype in mc.DTYPES:
                mlp = cls(*one, act=act, out_dtype=out_dtype, decode_kernel=decode_kernel)
                assert mlp.backend == "hip"
                for m in mc.DENSE_M:
                    x, want, bound = mc.dense_want(layer, tier, stored, m, out_dtype, act)
                    y = mlp(_dev(x, BF16))
                    what = (layer, tier, out_dtype, m)
                    if bound is None:
                        _equal(y, want.astype(np.float32), out_dtype, what)
                    else:
                        worst = max(worst, _within(y, want, bound, out_dtype, what))
                    n += 1
            if tier == "silu":
                print(f"dense, silu: stored={stored} decode_kernel={decode_kernel} {layer}: max error / bound = {worst:.4f}")
    print(f"dense: stored={stored} decode_kernel={decode_kernel}: {n} comparisons")
