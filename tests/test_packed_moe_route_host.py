"""CPU-only: the MoE router (packed.moe_route, MoERouting, MOE_ROUTINGS, PackedMoE.forward_logits; mtq_moe_route) as far as it goes
without a device.  The emulation against the two independent pieces of tests/moe_route_cases.py: want_select on the emulation's own
float32 scores, to the bit, and reference64 (ids where the decisive comparisons are clear, the score error under the bound); the
want-side's own promises on ties and special values; MoERouting and the presets; the layer; the binding's checks; the C entry's
refusals, which come back before a device is looked for (the pointers handed in are host addresses that no check may dereference).

  shapes    every (count, topk, tokens) of moe_route_cases.UNGROUPED up to count 384 and every row of GROUPED, each with its variant
            of score / bias / renormalize / eps / scale; the flagship (256, 8, 8 groups, 4 kept, top 2), (128, 8) and (384, 8) with
            every variant; a bias with negative entries under want_select.
  layer     the 5-expert 128 -> 96 -> 64 layer of test_packed_moe_host.py: forward_logits equals forward on moe_route's outputs."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import moe_route_cases as rc
from tests.inputs import gen, to_bf16_valued
from tests.test_capi_host import _load, _OnDevice, _StubLibrary
from tests.test_packed_moe_host import COUNT, K_IN, K_OUT, _experts

HEADER = Path(__file__).resolve().parents[1] / "include" / "mtq.h"
NEW = "mtq_moe_route"
INVALID, NO_DEVICE = -1, -3
HOST_MAX_COUNT = 384


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _emulated(x, topk, n_group, topk_group, group_top, variant, negative_bias=False):
    """The emulation on a case, checked against want_select on its own scores → (weights, ids, scores, bias)."""
    score, with_bias, renormalize, eps, scale = variant
    bias = rc.bias_of(x.shape[1], negative=negative_bias) if with_bias else None
    w, ids, s = packed.moe_route(x, topk, score, bias, n_group, topk_group, group_top, renormalize, eps, scale, backend="emulation",
                                 return_scores=True)
    assert (w.dtype, ids.dtype, s.dtype) == (np.float32, np.int32, np.float32)
    assert w.shape == ids.shape == (x.shape[0], topk) and s.shape == x.shape
    want_ids, want_w = rc.want_select(s, bias, topk, n_group, topk_group, group_top, renormalize, eps, scale)
    assert np.array_equal(ids, want_ids), np.flatnonzero((ids != want_ids).any(axis=1))[:8]
    assert np.array_equal(_words(w), _words(want_w)), np.argwhere(_words(w) != _words(want_w))[:4]
    assert all(np.unique(row).size == topk for row in ids) and ids.min() >= 0 and ids.max() < x.shape[1]
    two = packed.moe_route(x, topk, score, bias, n_group, topk_group, group_top, renormalize, eps, scale, backend="emulation")
    assert len(two) == 2 and np.array_equal(_words(two[0]), _words(w)) and np.array_equal(two[1], ids)
    return w, ids, s, bias


def _against_reference64(x, ids, s, bias, topk, n_group, topk_group, group_top, score, compare_ids=True):
    err = rc.check_against_reference64(ids, s, x, score, bias, topk, n_group, topk_group, group_top, what=(x.shape, topk, score),
                                       compare_ids=compare_ids)
    assert err <= rc.score_bound(x.shape[1]), (x.shape, score, err, rc.score_bound(x.shape[1]))


HOST_UNGROUPED = tuple(c for c in rc.ungrouped_cases() if c[0] <= HOST_MAX_COUNT)


@pytest.mark.parametrize("count,topk,n_group,topk_group,group_top,tokens,variant", HOST_UNGROUPED + tuple(rc.grouped_cases()))
def test_the_emulation_is_the_rule_on_its_scores_and_agrees_with_float64(count, topk, n_group, topk_group, group_top, tokens, variant):
    x = rc.logits_of(tokens, count)
    _w, ids, s, bias = _emulated(x, topk, n_group, topk_group, group_top, variant)
    _against_reference64(x, ids, s, bias, topk, n_group, topk_group, group_top, variant[0])


@pytest.mark.parametrize("variant", rc.VARIANTS)
@pytest.mark.parametrize("count,topk,n_group,topk_group,group_top", ((256, 8, 8, 4, 2), (128, 8, 1, 1, 2), (384, 8, 1, 1, 2)))
def test_every_variant_on_the_emulation(count, topk, n_group, topk_group, group_top, variant):
    x = rc.logits_of(67, count, seed=1)
    w, ids, s, bias = _emulated(x, topk, n_group, topk_group, group_top, variant)
    _against_reference64(x, ids, s, bias, topk, n_group, topk_group, group_top, variant[0], compare_ids=rc.ids_comparable(count, variant))
    score, _with_bias, renormalize, eps, scale = variant
    picked = np.take_along_axis(s, ids.astype(np.int64), axis=1).astype(np.float64)
    want = picked / (picked.sum(axis=1, keepdims=True) + eps) * scale if renormalize else picked * scale
    assert np.allclose(w, want, rtol=1e-5, atol=0)        # the weights are what the models compute, to float32's precision
    if variant[1]:                                        # a bias with negative entries: the rule holds all the same
        _emulated(x, topk, n_group, topk_group, group_top, variant, negative_bias=True)


def test_every_group_kept_is_the_ungrouped_result():
    x = rc.logits_of(67, 256)
    bias = rc.bias_of(256)
    s = packed.moe_route(x, 8, "sigmoid", bias, backend="emulation", return_scores=True)[2]
    assert all(np.array_equal(a, b) for a, b in zip(rc.want_select(s, bias, 8, 8, 8, 2), rc.want_select(s, bias, 8)))
    grouped = packed.moe_route(x, 8, "sigmoid", bias, 8, 8, 2, backend="emulation")
    flat = packed.moe_route(x, 8, "sigmoid", bias, backend="emulation")
    assert np.array_equal(grouped[1], flat[1]) and np.array_equal(_words(grouped[0]), _words(flat[0]))


def test_the_want_side_keeps_its_promises_on_ties_and_special_values():
    """What the GPU file's tie and special-value cases rest on, asserted on want_select alone."""
    s = np.full((1, 32), 0.25, dtype=np.float32)
    assert rc.want_select(s, None, 5)[0].tolist() == [[0, 1, 2, 3, 4]]                          # all equal: the lowest ids
    assert rc.want_select(s, None, 6, 4, 2, 2)[0].tolist() == [[0, 1, 2, 3, 4, 5]]              # the first experts of the first groups
    assert rc.want_select(s, None, 16, 4, 2, 2)[0].tolist() == [list(range(16))]
    s = np.array([[0.5, np.nan, -0.0, 0.0, -np.inf, 0.75]], dtype=np.float32)
    assert rc.want_select(s, None, 6, renormalize=False)[0].tolist() == [[5, 0, 2, 3, 1, 4]]     # -0 ties with +0, NaN with -Inf
    ids, w = rc.want_select(np.array([[0.25, 0.5, 0.125]], dtype=np.float32), np.array([0.5, 0, 0], dtype=np.float32), 2, scale=2.0)
    assert ids.tolist() == [[0, 1]] and np.allclose(w, [[2 / 3, 4 / 3]], rtol=1e-6, atol=0)     # the weights take the score, not the key
    g = np.array([[0.9, 0.0, 0.5, 0.5, 0.6, 0.2, 0.1, 0.1]], dtype=np.float32)                  # groups of two: 0.9 | 1.0 | 0.8 | 0.2
    assert rc.want_select(g, None, 2, 4, 1, 2)[0].tolist() == [[2, 3]] and rc.want_select(g, None, 2, 4, 1, 1)[0].tolist() == [[0, 1]]
    assert rc.want_select(g, None, 3, 4, 2, 2)[0].tolist() == [[0, 2, 3]]


def test_the_emulation_on_ties_masks_and_bad_tokens():
    count, K = 64, 6
    x = rc.logits_of(9, count).copy()
    x[1] = 0.5                                            # all equal
    x[2, :] = np.where(np.arange(count) % 2 == 0, -np.inf, x[2])               # half masked: fewer than count - K
    x[3, 3:] = -np.inf                                    # three experts left: more than count - K masked
    x[4, 7], x[5, 9], x[6] = np.nan, np.inf, -np.inf
    x[7] = 25.0                                           # sigmoid saturation
    clean = [0, 1, 2, 3, 7, 8]
    for score in ("softmax", "sigmoid"):
        for n_group, topk_group in ((1, 1), (8, 4)):
            w, ids, s = packed.moe_route(x, K, score, None, n_group, topk_group, 2, backend="emulation", return_scores=True)
            want_ids, want_w = rc.want_select(s, None, K, n_group, topk_group, 2)
            assert np.array_equal(ids, want_ids) and np.array_equal(_words(w)[clean], _words(want_w)[clean])
            assert all(np.unique(row).size == K for row in ids) and ids.min() >= 0 and ids.max() < count
            first = list(range(K)) if n_group == 1 else [0, 1, 2, 3, 4, 5]
            assert ids[1].tolist() == first
            assert (s[2, ::2] == 0).all() and not np.signbit(s[2, ::2]).any() and (ids[2] % 2 == 1).all()      # a masked expert scores +0
            assert set(ids[3, :3].tolist()) == {0, 1, 2} and (w[3, 3:] == 0).all()
            cw, cids = packed.moe_route(x[clean], K, score, None, n_group, topk_group, 2, backend="emulation")
            assert np.array_equal(cids, ids[clean]) and np.array_equal(_words(cw), _words(w[clean]))
            if score == "sigmoid":
                assert (s[7] == 1).all() and ids[7].tolist() == first


def test_leading_dimensions_tensors_and_bf16():
    x = rc.logits_of(10, 60)
    bias = rc.bias_of(60)
    w, ids, s = packed.moe_route(x, 5, "sigmoid", bias, return_scores=True)
    w3, ids3, s3 = packed.moe_route(torch.from_numpy(x.copy()).reshape(2, 5, 60), 5, "sigmoid", torch.from_numpy(bias.copy()), return_scores=True)
    assert isinstance(w3, torch.Tensor) and (w3.dtype, ids3.dtype, s3.dtype) == (torch.float32, torch.int32, torch.float32)
    assert tuple(w3.shape) == tuple(ids3.shape) == (2, 5, 5) and tuple(s3.shape) == (2, 5, 60)
    assert np.array_equal(_words(w3.numpy().reshape(10, 5)), _words(w)) and np.array_equal(ids3.numpy().reshape(10, 5), ids)
    xb = torch.from_numpy(to_bf16_valued(x * 1.37)).to(torch.bfloat16)
    got = packed.moe_route(xb, 5, "softmax", return_scores=True)
    same = packed.moe_route(xb.float(), 5, "softmax", return_scores=True)
    assert all(torch.equal(a, b) for a, b in zip(got, same))                    # a bf16 logit is widened exactly
    one = packed.moe_route(x[0], 5)
    assert one[0].shape == one[1].shape == (5,)


def test_routing_parameters_are_checked():
    for kw, match in (({"topk": 0}, "topk must be"), ({"topk": 65}, "topk must be"), ({"topk": 2.0}, "topk must be"), ({"topk": True}, "topk must be"),
                      ({"topk": 2, "score": "tanh"}, "score must be"), ({"topk": 2, "n_group": 0}, "n_group must be"),
                      ({"topk": 2, "n_group": 65}, "n_group must be"), ({"topk": 2, "n_group": 4, "topk_group": 5}, "topk_group must be"),
                      ({"topk": 2, "topk_group": 0}, "topk_group must be"), ({"topk": 2, "group_top": 3}, "group_top must be"),
                      ({"topk": 2, "group_top": 0}, "group_top must be"), ({"topk": 2, "renormalize": 1}, "renormalize must be"),
                      ({"topk": 2, "eps": float("nan")}, "eps must be"), ({"topk": 2, "scale": float("inf")}, "scale must be"),
                      ({"topk": 2, "scale": 1e39}, "scale must be"), ({"topk": 2, "eps": "0"}, "eps must be")):
        with pytest.raises(hb.MtqError, match=match):
            packed.MoERouting(**kw)
    r = packed.MoERouting(topk=8, n_group=8, topk_group=4)
    with pytest.raises(Exception):
        r.topk = 4                                        # frozen
    r.check_count(256)
    for routing, count, match in ((r, 100, "multiple of n_group"), (r, 8, "at most topk_group"), (r, 0, "count must be"),
                                  (r, 4104, "count must be"), (packed.MoERouting(topk=9), 8, "topk must be at most count"),
                                  (packed.MoERouting(topk=9, n_group=8, topk_group=2, group_top=1), 32, "at most topk_group"),
                                  (packed.MoERouting(topk=1, n_group=8, topk_group=2), 8, "group_top = 2 must be at most")):
        with pytest.raises(hb.MtqError, match=match):
            routing.check_count(count)
    packed.MoERouting(topk=64, n_group=64, topk_group=64, group_top=1).check_count(4096)         # the limits themselves pass
    x = rc.logits_of(3, 8)
    for bad, match in ((x.astype(np.float64), "bfloat16 or float32"), (x[:0], "at least one token"), (np.float32(1.0), "logits must be")):
        with pytest.raises(hb.MtqError, match=match):
            packed.moe_route(bad, 2)
    with pytest.raises(hb.MtqError, match=r"bias must be \(8,\)"):
        packed.moe_route(x, 2, bias=np.zeros(7, dtype=np.float32))
    with pytest.raises(hb.MtqError, match="backend must be"):
        packed.moe_route(x, 2, backend="cuda")
    with pytest.raises(hb.MtqError, match="topk must be at most count"):
        packed.moe_route(x, 9)


def test_the_presets_are_the_public_configurations():
    R = packed.MOE_ROUTINGS
    assert set(R) == {"mixtral", "qwen3-moe", "deepseek-v2", "deepseek-v3"} and all(isinstance(r, packed.MoERouting) for r in R.values())
    assert (R["mixtral"].score, R["mixtral"].topk, R["mixtral"].renormalize, R["mixtral"].n_group) == ("softmax", 2, True, 1)
    assert (R["qwen3-moe"].score, R["qwen3-moe"].topk, R["qwen3-moe"].renormalize) == ("softmax", 8, True)
    v2, v3 = R["deepseek-v2"], R["deepseek-v3"]
    assert (v2.score, v2.group_top, v2.renormalize, v2.n_group, v2.topk_group, v2.topk) == ("softmax", 1, False, 8, 3, 6)
    assert (v3.score, v3.n_group, v3.topk_group, v3.group_top, v3.renormalize, v3.eps, v3.scale, v3.topk, v3.expects_bias) == \
        ("sigmoid", 8, 4, 2, True, 1e-20, 2.5, 8, True)
    with pytest.raises(TypeError):
        R["mine"] = v3                                    # read-only
    R["mixtral"].check_count(8), R["qwen3-moe"].check_count(128), v2.check_count(160), v3.check_count(256)


def test_forward_logits_is_route_then_forward_on_the_emulation():
    gates, ups, downs = _experts()
    T = 11
    rng = np.random.default_rng(21)
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", 4, (T, K_IN)) * 50)).to(torch.bfloat16)
    base = torch.from_numpy(to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))).to(torch.bfloat16)
    logits = torch.from_numpy(rng.standard_normal((T, COUNT)).astype(np.float32))
    bias = torch.from_numpy((rng.integers(0, 64, size=COUNT) / 256).astype(np.float32))
    routings = (packed.MoERouting(topk=2), packed.MoERouting(topk=3, score="sigmoid", renormalize=True, eps=1e-20, scale=2.5, expects_bias=True),
                "mixtral")
    for router in routings:
        r = packed.MOE_ROUTINGS[router] if isinstance(router, str) else router
        b = bias if r.expects_bias else None
        for logit in (logits, logits.to(torch.bfloat16)):
            moe = packed.PackedMoE(gates, ups, downs, backend="emulation", router=router)
            assert moe.router == r
            w, ids = packed.moe_route(logit, r.topk, r.score, b, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale)
            assert isinstance(w, torch.Tensor) and tuple(ids.shape) == (T, r.topk)
            for bs in (None, base):
                want = moe(x, ids, w, base=bs)
                got = moe.forward_logits(x, logit, bias=b, base=bs)
                assert got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))
        y3 = moe.forward_logits(x[:10].reshape(2, 5, K_IN), logits[:10].reshape(2, 5, COUNT), bias=b)
        assert tuple(y3.shape) == (2, 5, K_OUT)
        assert torch.equal(y3.reshape(10, K_OUT).view(torch.int16), moe.forward_logits(x[:10], logits[:10], bias=b).view(torch.int16))
        assert tuple(moe.forward_logits(x[:0], logits[:0], bias=b).shape) == (0, K_OUT)
    moe = packed.PackedMoE(gates, ups, downs, backend="emulation", router=routings[1])
    with pytest.raises(hb.MtqError, match="needs the model's float32"):
        moe.forward_logits(x, logits)
    with pytest.raises(hb.MtqError, match="router_logits must be"):
        moe.forward_logits(x, logits[:, :4], bias=bias)
    with pytest.raises(hb.MtqError, match="forward_logits needs a router"):
        packed.PackedMoE(gates, ups, downs, backend="emulation").forward_logits(x, logits)
    for bad, match in (("llama", "router must be"), (8, "router must be"), (packed.MoERouting(topk=6), "topk must be at most count"),
                       ("deepseek-v3", "topk must be at most count"), (packed.MoERouting(topk=2, n_group=2), "multiple of n_group")):
        with pytest.raises(hb.MtqError, match=match):
            packed.PackedMoE(gates, ups, downs, backend="emulation", router=bad)


# ----------------------------------------------------------------------------- the binding and the C entry

def test_the_entry_is_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    assert re.search(rf"\b{NEW}\s*\(", text)
    assert hb.SIGNATURES[NEW] == ("i", "pilllliplliiddplplplp", True) and NEW in hb.OPTIONAL_EXPORTS and NEW in hb.EXPORTS
    assert getattr(hb.lib(), NEW) is not None and hb.MOE_ROUTE == (NEW,) and hb._has(hb.MOE_ROUTE)
    assert NEW not in hb.MOE and hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143
    for const, value in (("MTQ_MOE_MAX_GROUPS", hb.MOE_MAX_GROUPS),):
        assert re.search(rf"#define {const} {value}\b", text), const
    assert re.search(r"MTQ_ROUTE_SOFTMAX = 0, MTQ_ROUTE_SIGMOID = 1", text) and (hb.ROUTE_SOFTMAX, hb.ROUTE_SIGMOID) == (0, 1)
    assert packed.MOE_MAX_GROUPS == hb.MOE_MAX_GROUPS == 64
    assert (rc.REG_WAVES, rc.REG_MAX_COUNT, rc.MAX_BLOCKS) == (4, 256, 2048)
    source = (HEADER.parents[1] / "quantization_analysis_amd" / "csrc" / "mtq_moe_route.hip").read_text(encoding="utf-8")
    for name, value in (("kRouteRegWaves", rc.REG_WAVES), ("kRouteRegMaxCount", rc.REG_MAX_COUNT), ("kRouteMaxBlocks", rc.MAX_BLOCKS)):
        assert re.search(rf"constexpr int {name} = {value};", source), name


def test_a_build_without_the_entry_still_loads_and_nothing_stands_in(monkeypatch):
    stub = _StubLibrary(143, missing=(NEW,))
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_moe_combine.argtypes is not None and hb.has_moe() and not hb._has(hb.MOE_ROUTE)
    with pytest.raises(hb.MtqError, match="rebuild"):
        hb._entry(NEW)
    x = rc.logits_of(3, 8)
    with pytest.raises(hb.MtqError, match="mtq_moe_route.*lacks.*rebuild it from this tree"):
        packed.moe_route(x, 2, backend="hip")
    assert packed.moe_route(x, 2, backend="emulation")[1].shape == (3, 2)      # the emulation needs no library


def test_the_geometry_the_gpu_tests_assert():
    assert [rc.route_path(c) for c in (1, 64, 65, 128, 129, 256, 257, 4096)] == [(1, 4), (1, 4), (2, 4), (2, 4), (4, 4), (4, 4), (0, 1), (0, 1)]
    assert rc.route_grid(67, 8) == (17, 1) and rc.route_grid(8192, 8) == (2048, 1) and rc.route_grid(8195, 8) == (2048, 2)
    assert rc.route_grid(2048, 257) == (2048, 1) and rc.route_grid(2051, 257) == (2048, 2) and rc.route_grid(1, 1) == (1, 1)
    assert abs(rc.score_bound(4096) - 2.6e-6) < 0.1e-6 and 11 * rc.score_bound(4096) < rc.GAP < 12.5 * rc.score_bound(4096)   # about 6 x twice


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def test_route_refuses_before_a_device():
    fn = hb._entry(NEW)
    _buf, p = _aligned()

    def call(logits=p, dtype=hb.DTYPE_F32, ld=256, T=7, count=256, K=8, score=hb.ROUTE_SIGMOID, bias=p, n_group=8, topk_group=4, group_top=2,
             renorm=1, eps=1e-20, scale=2.5, ids=p, ld_ids=8, w=p, ld_w=8, scores=p, ld_scores=256):
        return fn(logits, dtype, ld, T, count, K, score, bias, n_group, topk_group, group_top, renorm, eps, scale, ids, ld_ids, w, ld_w, scores,
                  ld_scores, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in hb.lib().mtq_last_error().decode(), hb.lib().mtq_last_error().decode()

    for name in ("logits", "ids", "w"):
        refused("null argument", **{name: None})
    refused("logits_dtype", dtype=2)
    refused("score must be", score=2)
    refused("score must be", score=-1)
    refused("renormalize must be", renorm=2)
    refused("tokens must be positive", T=0)
    refused("tokens must be positive", T=-3)
    refused("tokens must be below 2^31", T=2 ** 31)
    refused("count must be", count=0, n_group=1, topk_group=1)
    refused("count must be", count=4097, ld=4097, ld_scores=4097, n_group=1, topk_group=1)
    refused("topk must be", K=0)
    refused("topk must be", K=65, ld_ids=65, ld_w=65)
    refused("topk must be", count=4, K=5, ld=4, n_group=1, topk_group=1)
    refused("n_group must be", n_group=0)
    refused("n_group must be", n_group=65)
    refused("multiple of n_group", n_group=7)
    refused("topk_group must be", topk_group=0)
    refused("topk_group must be", topk_group=9)
    refused("at most topk_group * count / n_group", count=16, ld=16, ld_scores=16, n_group=8, topk_group=3, K=8)
    refused("group_top must be 1 or 2", group_top=0)
    refused("group_top must be 1 or 2", group_top=3)
    refused("group_top must be at most", count=8, ld=8, ld_scores=8, n_group=8, topk_group=8, K=8, group_top=2)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        refused("eps and scale must be finite", eps=bad)
        refused("eps and scale must be finite", scale=bad)
    refused("ld_logits < count", ld=255)
    refused("ld_ids < topk", ld_ids=7)
    refused("ld_w < topk", ld_w=7)
    refused("ld_scores < count", ld_scores=255)
    refused("not aligned to its type", logits=p + 2)
    refused("not aligned to its type", logits=p + 1, dtype=hb.DTYPE_BF16)
    refused("not aligned to its type", ids=p + 2)
    refused("not aligned to its type", w=p + 1)
    refused("not aligned to its type", bias=p + 2)
    refused("not aligned to its type", scores=p + 3)
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert call() == NO_DEVICE and call(bias=None, scores=None, ld_scores=0) == NO_DEVICE
        assert call(logits=p + 2, dtype=hb.DTYPE_BF16, ld=300, ld_ids=11, ld_w=9, ld_scores=257) == NO_DEVICE
        assert call(count=4096, ld=4096, ld_scores=4096, K=64, ld_ids=64, ld_w=64, n_group=64, topk_group=64, group_top=1) == NO_DEVICE
        assert call(count=1, K=1, n_group=1, topk_group=1, group_top=1, T=2 ** 31 - 1) == NO_DEVICE


def test_the_binding_checks_its_operands_before_a_device():
    x = _OnDevice(torch.zeros((7, 16)))
    with pytest.raises(hb.MtqError, match="2-D"):
        hb.moe_route(_OnDevice(torch.zeros((7,))), 2)
    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.moe_route(_OnDevice(torch.zeros((7, 32))[:, ::2]), 2)
    with pytest.raises(hb.MtqError, match="bfloat16 or float32"):
        hb.moe_route(_OnDevice(torch.zeros((7, 16), dtype=torch.float16)), 2)
    with pytest.raises(hb.MtqError, match="device tensor"):
        hb.moe_route(torch.zeros((7, 16)), 2)
    with pytest.raises(hb.MtqError, match="score must be one of"):
        hb.moe_route(x, 2, score="tanh")
    with pytest.raises(hb.MtqError, match="must be positive"):
        hb.moe_route(x, 0)
    with pytest.raises(hb.MtqError, match="bias must"):
        hb.moe_route(x, 2, bias=_OnDevice(torch.zeros((16,), dtype=torch.float64)))
    with pytest.raises(hb.MtqError, match="bias must have count = 16"):
        hb.moe_route(x, 2, bias=_OnDevice(torch.zeros((17,))))
    ids, w, s = (_OnDevice(torch.zeros((7, 2), dtype=torch.int32)), _OnDevice(torch.zeros((7, 2))), _OnDevice(torch.zeros((7, 16))))
    with pytest.raises(hb.MtqError, match=r"out_ids must be a torch.int32 \(7, 2\)"):
        hb.moe_route(x, 2, out_ids=_OnDevice(torch.zeros((7, 2), dtype=torch.int64)), out_weights=w, out_scores=s)
    with pytest.raises(hb.MtqError, match=r"out_weights must be a torch.float32 \(7, 2\)"):
        hb.moe_route(x, 2, out_ids=ids, out_weights=_OnDevice(torch.zeros((7, 3))), out_scores=s)
    with pytest.raises(hb.MtqError, match=r"out_scores must be a torch.float32 \(7, 16\)"):
        hb.moe_route(x, 2, out_ids=ids, out_weights=w, out_scores=_OnDevice(torch.zeros((7, 32))[:, ::2]))
