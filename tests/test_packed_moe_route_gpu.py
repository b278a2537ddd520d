"""GPU: the MoE router kernels of csrc/mtq_moe_route.hip (mtq_moe_route) and packed.moe_route / PackedMoE.forward_logits on them.

The want-side is never the code under test (tests/moe_route_cases.py, which the host file draws from too): want_select, the
contract's rule in NumPy float32 on the scores the kernel emitted, must give the kernel's ids and weight words for every token of
every case, and a second call without `scores` must give the same words; reference64, the routing in float64 from the logits, must
give the same ids wherever the decisive comparisons are at least 2^-15 apart (at least 90 % of a case's tokens, asserted on the
want-side), and the emitted scores must be within the stated bound of its scores.  Everything pinned is compared as integer words.
Where a case is there for a kernel or a trip of the token loop, the test derives it from the shape with the host code's arithmetic
(moe_route_cases.route_path, route_grid) and asserts it.

  shapes    (count, topk) = (1, 1), (2, 1), (8, 2), (8, 8): everything selected, (60, 5): ragged lanes, (64, 6) | (65, 3): one and two
            experts a lane, (128, 8) | (129, 8): two and four, (256, 8) | (257, 8): the register kernels' last count and the LDS
            kernel's first, (384, 8), (4096, 64): both limits; grouped (256, 8, 8 groups, 4 kept, top 2): the flagship,
            (160, 6, 8, 3, top 1), (320, 8, 64, 8, top 2): the LDS kernel with a lane a group, (64, 4, 64, 4, top 1): groups of one
            expert, (32, 8, 4, 2, top 2): topk = every expert of the kept groups, (256, 8, 8, 8, top 2): every group kept, which equals
            the ungrouped result; n_group no power of two, where the lanes of groups n_group .. P - 1 (P the power of two at or above
            n_group) are idle and must stay out of kept_groups' ballot and butterfly: (96, 4, 3 groups, 2 kept), (60, 6, 6, 3),
            (240, 8, 12, 5), (384, 8, 24, 6) and (330, 8, 33, 8) on the LDS kernel, (120, 6, 5, 2), (192, 8, 48, 12); 1, 3, 5 or 67
            tokens, so that a workgroup's last wave is ragged.  Each with one variant of
            score / bias / renormalize / eps / scale; the flagship, (128, 8) and (384, 8) with every variant and a negative bias.
  grid      8195 tokens of 8 experts and 2051 tokens of 257: one token past 2048 workgroups' first pass and more.
  bf16      any values at 8, 256 (flat and grouped) and 384 experts: the words of the run on the same values widened to float32.
  views     logits a view of a wider buffer, and starting at an unaligned element; ids, weights and scores pitched views of sentinel
            buffers with sentinel rows behind them.
  special   all logits equal; pairs of equal logits straddling rank K; sigmoid saturation; experts masked at -Inf, fewer and more
            than count - K of them; tokens holding NaN, +Inf and all -Inf among clean tokens; ungrouped, 8 groups of 256 experts, and
            12 groups (5 kept) of a 240-expert copy of the same rows.
  layer     5 experts, 128 -> 96 -> 64: forward_logits equals forward on the route's outputs to the bit, T = 37 and T = 3, both
            `stored` values, with a base, leading dimensions (2, 5); nothing is read back.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_route_cases as rc
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL


def _words(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _run(x_dev, bias, topk, n_group, topk_group, group_top, variant):
    """The kernel on a case, checked against want_select on its own scores and against a call without scores → NumPy (ids, w, scores)."""
    score, _with_bias, renormalize, eps, scale = variant
    T, count = x_dev.shape
    ids_d, w_d, s_d = hb.moe_route(x_dev, topk, score, _dev(bias), n_group, topk_group, group_top, renormalize, eps, scale, return_scores=True)
    assert (ids_d.dtype, w_d.dtype, s_d.dtype) == (torch.int32, torch.float32, torch.float32)
    assert tuple(ids_d.shape) == tuple(w_d.shape) == (T, topk) and tuple(s_d.shape) == (T, count)
    ids, w, s = ids_d.cpu().numpy(), w_d.cpu().numpy(), s_d.cpu().numpy()
    assert ids.min() >= 0 and ids.max() < count and all(np.unique(row).size == topk for row in ids), "ids repeat or leave [0, count)"
    want_ids, want_w = rc.want_select(s, bias, topk, n_group, topk_group, group_top, renormalize, eps, scale)
    assert np.array_equal(ids, want_ids), np.flatnonzero((ids != want_ids).any(axis=1))[:8]
    fine = np.isfinite(want_w).all(axis=1)                # a token with a NaN score: its weights may be any words
    assert np.array_equal(_words(w)[fine], _words(want_w)[fine]), np.argwhere(_words(w) != _words(want_w))[:4]
    ids2, w2, none = hb.moe_route(x_dev, topk, score, _dev(bias), n_group, topk_group, group_top, renormalize, eps, scale)
    assert none is None and torch.equal(ids2, ids_d) and torch.equal(w2.view(torch.int32), w_d.view(torch.int32)), "a call without scores differs"
    return ids, w, s


def _case(x, topk, n_group, topk_group, group_top, variant, negative_bias=False, compare_ids=True):
    count = x.shape[1]
    bias = rc.bias_of(count, negative=negative_bias) if variant[1] else None
    ids, w, s = _run(_dev(x), bias, topk, n_group, topk_group, group_top, variant)
    err = rc.check_against_reference64(ids, s, x, variant[0], bias, topk, n_group, topk_group, group_top, what=(x.shape, topk, variant),
                                       compare_ids=compare_ids and not negative_bias)
    print(f"scores against float64: count {count} {variant[0]}: max relative error {err:.3e}, bound {rc.score_bound(count):.3e}")
    assert err <= rc.score_bound(count), (x.shape, variant, err, rc.score_bound(count))
    return ids, w, s, bias


@pytest.mark.parametrize("count,topk,n_group,topk_group,group_top,tokens,variant", tuple(rc.ungrouped_cases()) + tuple(rc.grouped_cases()))
def test_route_is_the_rule_on_its_scores_and_agrees_with_float64(count, topk, n_group, topk_group, group_top, tokens, variant):
    per, waves = rc.route_path(count)
    assert per == {1: 1, 2: 1, 8: 1, 60: 1, 64: 1, 65: 2, 128: 2, 129: 4, 160: 4, 256: 4, 257: 0, 320: 0, 384: 0, 4096: 0, 32: 1,
                   96: 2, 120: 2, 192: 4, 240: 4, 330: 0}[count]
    assert rc.route_grid(tokens, count) == (-(-tokens // waves), 1) and (waves == 1 or tokens % waves or tokens == 1)   # a ragged last workgroup
    if count == 4096:
        assert (count, topk) == (hb.MOE_MAX_EXPERTS, hb.MOE_MAX_TOPK) and not variant[1]          # the limits, without a bias
    x = rc.logits_of(tokens, count)
    ids, w, s, bias = _case(x, topk, n_group, topk_group, group_top, variant)
    score, _b, renormalize, eps, scale = variant
    pw, pids, ps = packed.moe_route(_dev(x), topk, score, _dev(bias), n_group, topk_group, group_top, renormalize, eps, scale, return_scores=True)
    assert pw.is_cuda and np.array_equal(pids.cpu().numpy(), ids) and np.array_equal(_words(pw.cpu().numpy()), _words(w))
    assert np.array_equal(_words(ps.cpu().numpy()), _words(s))
    if topk == count:
        assert all(sorted(row) == list(range(count)) for row in ids.tolist())                       # everything selected
    if (n_group, topk_group) == (8, 8):                   # every group kept: the ungrouped result
        flat = _run(_dev(x), bias, topk, 1, 1, 2, variant)
        assert np.array_equal(flat[0], ids) and np.array_equal(_words(flat[1]), _words(w))


@pytest.mark.parametrize("variant", rc.VARIANTS)
@pytest.mark.parametrize("count,topk,n_group,topk_group,group_top", ((256, 8, 8, 4, 2), (128, 8, 1, 1, 2), (384, 8, 1, 1, 2)))
def test_every_variant(count, topk, n_group, topk_group, group_top, variant):
    x = rc.logits_of(67, count, seed=1)
    ids, w, s, _bias = _case(x, topk, n_group, topk_group, group_top, variant, compare_ids=rc.ids_comparable(count, variant))
    _score, _with_bias, renormalize, eps, scale = variant
    picked = np.take_along_axis(s, ids.astype(np.int64), axis=1).astype(np.float64)
    want = picked / (picked.sum(axis=1, keepdims=True) + eps) * scale if renormalize else picked * scale
    assert np.allclose(w, want, rtol=1e-5, atol=0)
    if variant[1]:
        _case(x, topk, n_group, topk_group, group_top, variant, negative_bias=True)


@pytest.mark.parametrize("tokens,count,topk", ((8195, 8, 2), (2051, 257, 8)))
def test_route_strides_past_its_grid(tokens, count, topk):
    blocks, trips = rc.route_grid(tokens, count)
    _per, waves = rc.route_path(count)
    assert (blocks, trips) == (rc.MAX_BLOCKS, 2) and rc.route_grid(rc.MAX_BLOCKS * waves, count) == (rc.MAX_BLOCKS, 1)
    assert 0 < tokens - rc.MAX_BLOCKS * waves < waves or waves == 1                                   # the second pass is ragged
    x = np.tile(rc.logits_of(67, count, seed=2), (-(-tokens // 67), 1))[:tokens].copy()
    x[rc.MAX_BLOCKS * waves:] = x[rc.MAX_BLOCKS * waves:, ::-1]                                       # the tokens of the second pass: rows of their own
    variant = ("sigmoid", True, True, 1e-20, 2.5) if count == 8 else ("softmax", False, True, 0.0, 1.0)
    bias = rc.bias_of(count) if variant[1] else None
    ids, w, s = _run(_dev(x), bias, topk, 1, 1, 2, variant)
    want = rc.reference64(x[-67:], variant[0], bias, topk)
    clear = want[2] >= rc.GAP
    assert clear.mean() >= rc.QUALIFY and np.array_equal(ids[-67:][clear], want[0][clear])


@pytest.mark.parametrize("count,topk,n_group,topk_group", ((8, 2, 1, 1), (256, 8, 1, 1), (256, 8, 8, 4), (384, 8, 1, 1)))
def test_bf16_logits_are_widened_exactly(count, topk, n_group, topk_group):
    rng = np.random.default_rng(count + n_group)
    x = to_bf16_valued((rng.standard_normal((21, count)) * 3).astype(np.float32))
    x[0, 0], x[1, 1 % count] = -np.inf, 0.0
    xb = torch.from_numpy(x).to(torch.bfloat16).cuda()
    assert torch.equal(xb.float().cpu(), torch.from_numpy(x))
    for variant in (("softmax", False, True, 0.0, 1.0), ("sigmoid", True, True, 1e-20, 2.5)):
        bias = rc.bias_of(count) if variant[1] else None
        got = _run(xb, bias, topk, n_group, topk_group, 2, variant)
        same = _run(_dev(x), bias, topk, n_group, topk_group, 2, variant)
        assert np.array_equal(got[0], same[0]) and np.array_equal(_words(got[1]), _words(same[1])) and np.array_equal(_words(got[2]), _words(same[2]))


@pytest.mark.parametrize("count,topk,n_group,topk_group", ((60, 5, 1, 1), (256, 8, 8, 4), (320, 8, 64, 8)))
def test_views_and_bounds(count, topk, n_group, topk_group):
    T = 13
    variant = ("sigmoid", True, True, 1e-20, 2.5)
    x = rc.logits_of(T, count, seed=3)
    bias = rc.bias_of(count)
    want = _run(_dev(x), bias, topk, n_group, topk_group, 2, variant)
    score, _b, renormalize, eps, scale = variant
    for dtype in (torch.float32, torch.bfloat16):
        xt = torch.from_numpy(to_bf16_valued(x.copy()))
        ref = _run(xt.cuda(), bias, topk, n_group, topk_group, 2, variant) if dtype == torch.bfloat16 else want
        wide = torch.full((T + 2, count + 7), 3.5, dtype=dtype, device="cuda")          # large logits around the view: a misread shows
        src = xt if dtype == torch.bfloat16 else torch.from_numpy(x.copy())
        wide[1: 1 + T, 3: 3 + count] = src.to(dtype).cuda()
        view = wide[1: 1 + T, 3: 3 + count]
        assert view.data_ptr() % 16 != 0 and view.stride(0) == count + 7
        ids_buf = torch.full((T + 3, topk + 5), -7, dtype=torch.int32, device="cuda")
        w_buf = torch.full((T + 3, topk + 3), -7.0, dtype=torch.float32, device="cuda")
        s_buf = torch.full((T + 3, count + 9), -7.0, dtype=torch.float32, device="cuda")
        ids_v, w_v, s_v = ids_buf[1: 1 + T, 2: 2 + topk], w_buf[1: 1 + T, 1: 1 + topk], s_buf[1: 1 + T, 4: 4 + count]
        out = hb.moe_route(view, topk, score, _dev(bias), n_group, topk_group, 2, renormalize, eps, scale, out_ids=ids_v, out_weights=w_v,
                           out_scores=s_v)
        assert out[0].data_ptr() == ids_v.data_ptr() and out[2].data_ptr() == s_v.data_ptr()
        assert np.array_equal(ids_v.cpu().numpy(), ref[0]) and np.array_equal(_words(w_v.cpu().numpy()), _words(ref[1]))
        assert np.array_equal(_words(s_v.cpu().numpy()), _words(ref[2]))
        for buf, inner in ((ids_buf, ids_v), (w_buf, w_v), (s_buf, s_v)):
            mask = torch.ones_like(buf, dtype=torch.bool)
            mask[1: 1 + T, inner.storage_offset() % buf.stride(0): inner.storage_offset() % buf.stride(0) + inner.shape[1]] = False
            assert bool((buf[mask] == -7).all()), "something outside tokens x topk / tokens x count was written"


def test_ties_and_special_values():
    count, K = 256, 8
    x = rc.logits_of(12, count, seed=4).copy()
    x[1] = 0.5                                            # all equal
    order = np.argsort(-x[2])
    x[2, order[K]] = x[2, order[K - 1]]                   # a pair of equal logits straddling rank K
    x[2, order[K + 2]] = x[2, order[K + 1]]
    x[3] = np.where(np.arange(count) % 2 == 0, -np.inf, x[3])                  # half masked: fewer than count - K
    x[4, 5:] = -np.inf                                    # five experts left: more than count - K masked
    x[5, 7], x[6, 200], x[7] = np.nan, np.inf, -np.inf
    x[8] = np.where(np.arange(count) < 100, 20.0 + np.arange(count) % 7, x[8])     # sigmoid saturation: a hundred scores of 1.0f
    clean = [0, 1, 2, 3, 4, 8, 9, 10, 11]
    whole = x
    for score in ("softmax", "sigmoid"):
        for n_group, topk_group in ((1, 1), (8, 4), (12, 5)):
            variant = (score, False, True, 0.0, 1.0)
            x = whole[:, :240] if n_group == 12 else whole           # 12 groups of 20: a 240-expert copy of the same rows, 4 idle group slots
            ids, w, s = _run(_dev(x), None, K, n_group, topk_group, 2, variant)
            assert ids[1].tolist() == list(range(K))      # the first K experts (of the first topk_group groups: 32 an expert group)
            low, high = sorted((int(order[K - 1]), int(order[K])))
            assert n_group > 1 or (low in ids[2] and high not in ids[2])                              # the tie at rank K goes to the lower id
            assert (s[3, ::2] == 0).all() and not np.signbit(s[3, ::2]).any() and (ids[3] % 2 == 1).all()      # a masked expert scores +0
            assert set(ids[4, :5].tolist()) == set(range(5)) and ids[4, 5:].tolist() == [5, 6, 7] and (w[4, 5:] == 0).all()
            if score == "sigmoid":
                assert (s[8, :100] == 1).all() and ids[8].tolist() == list(range(K))
            cids, cw, cs = _run(_dev(x[clean]), None, K, n_group, topk_group, 2, variant)             # the clean tokens alone: the same words
            assert np.array_equal(cids, ids[clean]) and np.array_equal(_words(cw), _words(w[clean])) and np.array_equal(_words(cs), _words(s[clean]))
    for count2 in (8, 384):                               # the other kernels on bad tokens: ids distinct and in range (asserted in _run)
        y = rc.logits_of(6, count2, seed=5).copy()
        y[1, 0], y[2, count2 - 1], y[3] = np.nan, np.inf, -np.inf
        y[4] = 1.25
        for score in ("softmax", "sigmoid"):
            ids, _w, _s = _run(_dev(y), None, 4, 1, 1, 2, (score, False, True, 1e-20, 1.0))
            assert ids[4].tolist() == [0, 1, 2, 3]


# ----------------------------------------------------------------------------- the layer

COUNT, K_IN, HIDDEN, K_OUT = 5, 128, 96, 64


@functools.lru_cache(maxsize=None)
def _experts(stored):
    ws = [np.stack([gen("heavy_f32", seed + i, shape) for i in range(COUNT)]) for seed, shape in ((30, (HIDDEN, K_IN)), (40, (HIDDEN, K_IN)), (50, (K_OUT, HIDDEN)))]
    if stored == "transpose":                             # (k, n) experts: the ordinary packed tensors of the transposed weights
        ws = [np.ascontiguousarray(w.transpose(0, 2, 1)) for w in ws]
    maps = [np.stack([random_map(w.shape[1:], seed + i) for i in range(COUNT)]) for w, seed in zip(ws, (33, 43, 53))]
    return tuple(packed.pack_batch(torch.from_numpy(w).cuda(), m, backend="hip") for w, m in zip(ws, maps))


def _bits(t) -> np.ndarray:
    t = t.detach()
    return (t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)).cpu().numpy()


@pytest.mark.parametrize("stored", packed.MOE_STORED)
@pytest.mark.parametrize("T,decode_max_rows", ((37, None), (3, 64)))
def test_forward_logits_is_route_then_forward(T, decode_max_rows, stored):
    rng = np.random.default_rng(T)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", T, (T, K_IN)) * 50)).to(torch.bfloat16).cuda()
    base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))).to(torch.bfloat16).cuda()
    logits = torch.from_numpy(rng.standard_normal((T, COUNT)).astype(np.float32)).cuda()
    bias = torch.from_numpy((rng.integers(0, 64, size=COUNT) / 256).astype(np.float32)).cuda()
    for router in ("mixtral", packed.MoERouting(topk=3, score="sigmoid", eps=1e-20, scale=2.5, expects_bias=True)):
        r = packed.MOE_ROUTINGS[router] if isinstance(router, str) else router
        b = bias if r.expects_bias else None
        moe = packed.PackedMoE(*_experts(stored), out_dtype="float32", decode_max_rows=decode_max_rows, stored=stored, router=router)
        assert moe.backend == "hip" and moe.router == r
        for logit in (logits, logits.to(torch.bfloat16)):
            w, ids = packed.moe_route(logit, r.topk, r.score, b, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale)
            want_ids, want_w = rc.want_select(packed.moe_route(logit, r.topk, r.score, b, return_scores=True)[2].cpu().numpy(), None if b is None else
                                              b.cpu().numpy(), r.topk, 1, 1, 2, r.renormalize, r.eps, r.scale)
            assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(_words(w.cpu().numpy()), _words(want_w))
            for bs in (None, base):
                want = moe(x, ids, w, base=bs)
                got = moe.forward_logits(x, logit, bias=b, base=bs)
                assert tuple(got.shape) == (T, K_OUT) and np.array_equal(_bits(got), _bits(want)), (router, bs is None)
    if T == 37:                                           # leading dimensions
        y3 = moe.forward_logits(x[:10].reshape(2, 5, K_IN), logits[:10].reshape(2, 5, COUNT), bias=b, base=base[:10].reshape(2, 5, K_OUT))
        assert tuple(y3.shape) == (2, 5, K_OUT)
        assert np.array_equal(_bits(y3).reshape(10, K_OUT), _bits(moe.forward_logits(x[:10], logits[:10], bias=b, base=base[:10])))
        assert tuple(moe.forward_logits(x[:0], logits[:0], bias=b).shape) == (0, K_OUT)
        with pytest.raises(hb.MtqError, match="needs the model's float32"):
            moe.forward_logits(x, logits)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode is a prototype feature")
def test_forward_logits_reads_nothing_back():
    T = 37
    rng = np.random.default_rng(1)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", 3, (T, K_IN)) * 50)).to(torch.bfloat16).cuda()
    logits = torch.from_numpy(rng.standard_normal((T, COUNT)).astype(np.float32)).cuda()
    moe = packed.PackedMoE(*_experts("rows"), decode_max_rows=64, max_tokens=1, router="mixtral")
    calls = ((x, logits), (x[:3], logits[:3]))
    want = [_bits(moe.forward_logits(a, b)) for a, b in calls]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [moe.forward_logits(a, b) for a, b in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(np.array_equal(_bits(g), w_) for g, w_ in zip(got, want))
