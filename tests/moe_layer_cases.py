"""What tests/test_packed_moe_layer_exact_host.py and tests/test_packed_moe_layer_exact_gpu.py share: three MoE layers in both `stored`
orientations, their routings, and a float64 reference of the WHOLE layer that no code under test takes part in.  NumPy, the oracle
and the emulation only: no fixture, no device.

The exact tier: inputs on which every float32 operation of every route is exact in any order, so a kernel must EQUAL float64.

  x          integers, |x| <= 4.
  weights    integers in [-3, 3] times 2^-2, a different random_map over all four codes per expert and projection.  Ŵ is the oracle's
             (packed_cases.expected_bits), never unpack, and asserted to lie on the 2^-2 grid (bfp2 moves values, and stays on it).
  top-k w    from {-1, -0.5, 0, 0.25, 0.5, 1}: every product w * d is exact.
  base       None, or multiples of 2^-2 with |b| <= 16 (bf16 values too), no -0.0.
  act        "none".
  reference  per (token, expert): g = Ŵg x, u = Ŵu x, h = g * u (asserted to be a float32), h to bf16 by round-to-nearest-even,
             d = Ŵd h, d to bf16 when expert_dtype is bfloat16; y = base + sum of w_j d_j over the live slots; y to out_dtype.
  conditions each stage's sum of absolute terms divided by its granularity stays below 2^24, asserted before any code under test
             runs: sum|x||ŵ| / 2^-2 (the projections), sum|h||ŵd| / 2^-6 (the down projection), (|base| + sum|w||d|) / 2^-8 (the
             combine).  Every partial sum of every order is then a multiple of the granularity below 2^24 of them: a float32.
             A 2^-4 weight grid fails the down stage (2^25).  headroom() gives log2 of the largest quotients.

The rows are computed for EVERY (token, expert), a superset of the live slots: the conditions hold for any routing of these tokens,
and a routing only picks rows.

The bounded tier, for what act="none" cannot see (g * u is symmetric: gate and up exchanged is invisible above): act="silu",
heavy_f32 weights, x bf16-valued normal, top-k weights from moe_route under mixtral's routing and under deepseek-v3's (sigmoid, a
selection bias, renormalised, eps, scale; its groups cut down to the layer's expert count).  The reference is the recipe above with
silu.  The bound is derived, not measured, by composing the project's stated bounds, all per output element:

  B_h   |h - h64| for a float32 h: _silu_bound of tests/test_packed_glu_gpu.py.
  E_h   = B_h + 2^-9 (|h64| + B_h): h stored as bf16 (*).
  E_d   = E_h |Ŵd|ᵀ + (hidden + 2) 2^-24 (|ĥ| |Ŵd|ᵀ): the error of h through the down projection, and the linear bound of §A.6h
          on the float32 sums of the product itself (ĥ: the reference's bf16 h);
          + 2^-9 (|d64| + E_d) where expert_dtype is bfloat16 (*).
  E_y   = sum_j |w_j| E_d[j] + (K + 2) 2^-24 (|base| + sum_j |w_j| |d_j|): the rows' errors through the combine, and K products and
          K sums of float32;
          + 2^-9 (|y64| + E_y) where out_dtype is bfloat16 (*).

(*) A store to bf16 (_store_bf16).  The reference rounds its own value v to bf16 as well, and a float32 within E of v rounds, by
the monotonicity of rounding, to a bf16 between bf16(v - E) and bf16(v + E).  Where no rounding boundary lies within E of v that is
bf16(v) itself; where one does, a correct result may be the neighbour, a whole bf16 ulp (up to 2^-7 |v|) away, which E + 2^-9 (|v| + E)
does not always cover: the float64 emulation itself met it (y64 = -16.0625001 with E = 0.092, the float32 combine at -16.0624995:
-16.0 against -16.125, 1.009 of that term).  So the allowance of a store is the larger of the two,
max(E + 2^-9 (|v| + E), |bf16(v + E) - bf16(v)|, |bf16(v - E) - bf16(v)|): never less than the first form, and wider only where a
boundary lies inside the interval.

A condition on the want-side (silu_want(..., exchanged=True)): the reference with gate and up exchanged lies OUTSIDE the bound on at
least one output of every token that has a live slot, so a route that exchanged them cannot pass.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.moe_cases import _want_plan
from tests.packed_cases import expected_bits, random_map
from tests.test_packed_glu_gpu import _silu_bound, _silu64

LAYERS = {"even": (5, 128, 96, 64),                       # (count, k_in, hidden, k_out): the layer of DESIGN.md §A.6w
          "ragged": (3, 100, 76, 40),                     # both tile dimensions ragged, k and hidden no multiples of 8: element-wise X and h
          "long": (3, 256, 256, 40)}                      # eight tiles along both K: the library's own split is 2 in both decode stages
STORED = ("rows", "transpose")
ROUTINGS = ((3, 2), (5, 3), (32, 8), (37, 2), (130, 8))   # (T, K); (5, 3) on the ragged layer only, (3, 2) and (37, 2) on the long one
PAIRS = tuple((layer, T, K) for layer in ("even", "ragged") for T, K in ROUTINGS if layer == "ragged" or (T, K) != (5, 3)) + \
    (("long", 3, 2), ("long", 37, 2))
DECODE_MAX_ROWS = 256                                     # of every decode module of the GPU file: S = 256 is the last decode call
DTYPES = ("float32", "bfloat16")
BASES = (None, "bfloat16", "float32")
TOPK_WEIGHTS = (-1.0, -0.5, 0.0, 0.25, 0.5, 1.0)
W_GRID, DOWN_GRID, COMBINE_GRID = 2.0 ** -2, 2.0 ** -6, 2.0 ** -8
LIMIT = 2.0 ** 24
U24, BF16_HALF = 2.0 ** -24, 2.0 ** -9
MAP_SEEDS = (33, 43, 53)                                  # gate, up, down; + the expert's index
DENSE_M = (1, 5, 32, 33)                                  # PackedMLP: the skinny range and the first row past it
DENSE_EXPERT = 2


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def _bf16(a64: np.ndarray) -> np.ndarray:
    """float64 values that are float32s (or near: the bounded tier) → round-to-nearest-even bf16, as float64."""
    return to_bf16_valued(a64.astype(np.float32)).astype(np.float64)


def _store_bf16(v: np.ndarray, e: np.ndarray):
    """(bf16(v), the allowance behind the store) for a computed float32 within e of v: see (*) of the module's docstring."""
    r = _bf16(v)
    return r, np.maximum(e + BF16_HALF * (np.abs(v) + e), np.maximum(np.abs(_bf16(v + e) - r), np.abs(_bf16(v - e) - r)))


# ----------------------------------------------------------------------------- the layers

def _shapes(layer):
    count, k_in, hidden, k_out = LAYERS[layer]
    return (count, hidden, k_in), (count, hidden, k_in), (count, k_out, hidden)


@functools.lru_cache(maxsize=None)
def weights(layer, tier):
    """(gate, up, down) float32 (count, n, k): the same arrays for both orientations."""
    if tier == "exact":
        rng = np.random.default_rng(len(layer) + 7)
        return tuple(_frozen((rng.integers(-3, 4, size=s) * W_GRID).astype(np.float32)) for s in _shapes(layer))
    assert tier == "silu"
    return tuple(_frozen(np.stack([gen("heavy_f32", seed + i, s[1:]) for i in range(s[0])])) for seed, s in zip((30, 40, 50), _shapes(layer)))


@functools.lru_cache(maxsize=None)
def maps(layer, stored):
    """Per projection the (count, tiles, tiles) maps: over W's grid for "rows", over Wᵀ's for "transpose"."""
    got = tuple(np.stack([random_map((n, k) if stored == "rows" else (k, n), seed + i) for i in range(count)])
                for seed, (count, n, k) in zip(MAP_SEEDS, _shapes(layer)))
    assert all(np.unique(m).size == 4 for m in got)       # all four codes in every projection
    return got


@functools.lru_cache(maxsize=None)
def experts(layer, tier, stored, backend="emulation"):
    """(gate, up, down) lists of packed experts: pack_batch of W for "rows", pack_batch_transposed of the same W for "transpose"."""
    pack = packed.pack_batch if stored == "rows" else packed.pack_batch_transposed
    out = []
    for w, m in zip(weights(layer, tier), maps(layer, stored)):
        if backend != "emulation":
            import torch

            w = torch.from_numpy(np.array(w)).cuda()
        out.append(pack(w, m, backend=backend))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def what(layer, tier, stored):
    """(Ŵg, Ŵu, Ŵd) float64 (count, n, k) from the oracle: the quantisation of W by its map, or of Wᵀ by its map, transposed back."""
    out = []
    for w, m in zip(weights(layer, tier), maps(layer, stored)):
        if stored == "rows":
            q = np.stack([expected_bits(w[e], m[e]).view(np.float32) for e in range(w.shape[0])])
        else:
            q = np.stack([expected_bits(np.ascontiguousarray(w[e].T), m[e]).view(np.float32).T for e in range(w.shape[0])])
        q = q.astype(np.float64)
        if tier == "exact":
            assert np.array_equal(q / W_GRID, np.round(q / W_GRID)) and np.abs(q).max() <= 3 * W_GRID
        out.append(_frozen(q))
    return tuple(out)


# ----------------------------------------------------------------------------- the routings

def routing(T, K, count, seed=0) -> np.ndarray:
    """int64 ids (T, K).  Expert 2 is hot (seven slots in ten), the odd experts stay empty, one slot in twenty is -1 and one
    count + 3; token 0 names one expert twice, token 1 has no live slot at all."""
    other = count - 1 if count - 1 != 2 else 0
    pattern = np.array([2] * 7 + [0, other, -1] + [2] * 7 + [0, other, count + 3], dtype=np.int64)
    ids = np.random.default_rng(1000 * T + K + seed).permutation(pattern[np.arange(T * K) % pattern.size]).reshape(T, K)
    ids[0, :2] = other
    ids[1] = np.where(np.arange(K) % 2 == 0, -1, count + 3)
    return ids


def check_routing(ids, count) -> np.ndarray:
    """What every routing promises, on the want-side → the groups' sizes."""
    group_rows, _row_of, _src = _want_plan(ids, count)
    sizes = np.diff(group_rows)
    live = (ids >= 0) & (ids < count)
    assert (sizes == 0).any() and (ids == -1).any() and (ids == count + 3).any()
    assert ids[0, 0] == ids[0, 1] and live[0, :2].all() and not live[1].any() and live[2:].any()
    return sizes


@functools.lru_cache(maxsize=None)
def exact_inputs(layer, T, K):
    """(x (T, k_in) integers, ids int64 (T, K), w float32 (T, K), base float32 (T, k_out)) of a (layer, routing) pair."""
    count, k_in, _hidden, k_out = LAYERS[layer]
    rng = np.random.default_rng(100 * T + K + len(layer))
    x = rng.integers(-4, 5, size=(T, k_in)).astype(np.float32)
    ids = routing(T, K, count)
    w = rng.choice(np.array(TOPK_WEIGHTS, dtype=np.float32), size=(T, K))
    w[0, :2] = (0.5, -1.0)                                # the expert named twice: two different weights
    base = (rng.integers(-64, 65, size=(T, k_out)) * W_GRID).astype(np.float32) + np.float32(0)
    assert not np.signbit(base[base == 0]).any() and np.array_equal(to_bf16_valued(base), base) and np.abs(base).max() <= 16
    return _frozen(x), _frozen(ids), _frozen(w), _frozen(base)


# ----------------------------------------------------------------------------- the exact reference

@functools.lru_cache(maxsize=None)
def exact_rows(layer, stored, T, K):
    """(d float64 (T, count, k_out), (projection, down) quotients): every token through every expert, conditions asserted."""
    count, _k_in, hidden, k_out = LAYERS[layer]
    x = exact_inputs(layer, T, K)[0].astype(np.float64)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4
    wg, wu, wd = what(layer, "exact", stored)
    d = np.zeros((T, count, k_out))
    q_proj = q_down = 0.0
    rounded = False
    for e in range(count):
        g, u = x @ wg[e].T, x @ wu[e].T
        q_proj = max(q_proj, float((np.abs(x) @ np.abs(wg[e]).T).max()) / W_GRID, float((np.abs(x) @ np.abs(wu[e]).T).max()) / W_GRID)
        h = g * u
        assert np.array_equal(h.astype(np.float32).astype(np.float64), h) and np.abs(h).max() > 1.0
        hb = _bf16(h)
        rounded = rounded or not np.array_equal(hb, h)
        q_down = max(q_down, float((np.abs(hb) @ np.abs(wd[e]).T).max()) / DOWN_GRID)
        d[:, e] = hb @ wd[e].T
    assert q_proj < LIMIT and q_down < LIMIT, (layer, stored, T, K, q_proj, q_down)
    assert rounded                                        # some h loses bits on its way to bf16: a route that kept float32 differs
    assert np.array_equal(d / DOWN_GRID, np.round(d / DOWN_GRID))
    return _frozen(d), (q_proj, q_down)


def _combine64(d, ids, w, base):
    """(y64, sum of absolute terms): base + sum_j w_j d[t, ids[t, j]] over the live slots, in float64."""
    T, count, k_out = d.shape
    y = np.zeros((T, k_out)) if base is None else base.astype(np.float64).copy()
    mass = np.abs(y)
    rows = np.arange(T)
    for j in range(ids.shape[1]):
        e = ids[:, j].astype(np.int64)
        live = (e >= 0) & (e < count)
        term = np.where(live[:, None], d[rows, np.where(live, e, 0)], 0.0)
        y = y + w[:, j].astype(np.float64)[:, None] * term
        mass = mass + np.abs(w[:, j].astype(np.float64))[:, None] * np.abs(term)
    return y, mass


@functools.lru_cache(maxsize=None)
def exact_want(layer, stored, T, K, expert_dtype, out_dtype, with_base):
    """(y float32 (T, k_out), the combine's quotient): the layer's output, every value of it exact."""
    _x, ids, w, base = exact_inputs(layer, T, K)
    d = exact_rows(layer, stored, T, K)[0]
    if expert_dtype == "bfloat16":
        d = _bf16(d)
    y, mass = _combine64(d, ids, w, base if with_base else None)
    q = float(mass.max()) / COMBINE_GRID
    assert q < LIMIT, (layer, stored, T, K, q)
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y) and np.array_equal(y / COMBINE_GRID, np.round(y / COMBINE_GRID))
    live = ((ids >= 0) & (ids < LAYERS[layer][0])).any(axis=1)
    assert np.array_equal(y32[~live], base[~live] if with_base else np.zeros_like(y32[~live]))      # no live slot: base, or +0
    if out_dtype == "bfloat16":
        y32 = to_bf16_valued(y32)
    return _frozen(y32 + np.float32(0)), q


def headroom(layer, T, K):
    """log2 of the largest quotient of each stage over both orientations, expert types and bases: (projection, down, combine)."""
    proj = max(exact_rows(layer, s, T, K)[1][0] for s in STORED)
    down = max(exact_rows(layer, s, T, K)[1][1] for s in STORED)
    comb = max(exact_want(layer, s, T, K, e, "float32", True)[1] for s in STORED for e in DTYPES)
    return tuple(float(np.log2(v)) for v in (proj, down, comb))


def dense_want(layer, tier, stored, m, out_dtype, act):
    """One expert's MLP alone on the first m tokens of the (37, 2) inputs → (x (m, k_in), y float64 (m, k_out), bound or None)."""
    if tier == "exact":
        assert act == "none"
        x = exact_inputs(layer, 37, 2)[0][:m]
        y = exact_rows(layer, stored, 37, 2)[0][:m, DENSE_EXPERT]
        return x, (_bf16(y) if out_dtype == "bfloat16" else y), None
    assert act == "silu"
    x = silu_inputs(layer, 37, "mixtral")[0][:m]
    d, e_d = (a[:m, DENSE_EXPERT] for a in silu_rows(layer, stored, 37, "mixtral"))
    if out_dtype == "bfloat16":
        return (x,) + _store_bf16(d, e_d)
    return x, d, e_d


# ----------------------------------------------------------------------------- the bounded tier

SILU_CASES = (("even", 3, "mixtral"), ("even", 37, "mixtral"), ("even", 130, "mixtral"), ("even", 40, "deepseek-v3"),
              ("ragged", 5, "deepseek-v3"), ("ragged", 37, "mixtral"), ("ragged", 130, "deepseek-v3"), ("long", 37, "deepseek-v3"))


def router(layer, name) -> packed.MoERouting:
    """mixtral's routing as it is; deepseek-v3's with one expert a group, as many groups as the layer has experts."""
    count = LAYERS[layer][0]
    if name == "mixtral":
        return packed.MOE_ROUTINGS["mixtral"]
    assert name == "deepseek-v3"
    keep = 3 if count == 5 else 2
    r = dataclasses.replace(packed.MOE_ROUTINGS["deepseek-v3"], topk=keep, n_group=count, topk_group=keep, group_top=1)
    r.check_count(count)
    assert r.expects_bias and r.score == "sigmoid" and r.renormalize
    return r


@functools.lru_cache(maxsize=None)
def silu_inputs(layer, T, name):
    """(x (T, k_in) bf16-valued, logits float32 (T, count), bias float32 (count,) or None, base float32 bf16-valued (T, k_out),
    ids int32 (T, K), w float32 (T, K)): ids and w from the emulated moe_route; expert 2's logit is raised, so its group is long."""
    count, k_in, _hidden, k_out = LAYERS[layer]
    rng = np.random.default_rng(10 * T + len(layer) + len(name))
    x = to_bf16_valued(gen("normal_f32", 3 * T + len(name), (T, k_in)) * 50)
    logits = rng.standard_normal((T, count)).astype(np.float32)
    logits[:, 2] += np.float32(2)
    r = router(layer, name)
    bias = (rng.integers(0, 64, size=count) / 256.0).astype(np.float32) if r.expects_bias else None
    base = to_bf16_valued(rng.standard_normal((T, k_out)).astype(np.float32))
    w, ids = packed.moe_route(logits, r.topk, r.score, bias, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale, backend="emulation")
    assert ids.shape == (T, r.topk) and w.dtype == np.float32
    return _frozen(x), _frozen(logits), None if bias is None else _frozen(bias), _frozen(base), _frozen(ids), _frozen(w)


@functools.lru_cache(maxsize=None)
def silu_rows(layer, stored, T, name, exchanged=False):
    """(d64, E_d) float64 (T, count, k_out) for float32 expert rows: every token through every expert; `exchanged`: gate and up exchanged."""
    count, _k_in, hidden, k_out = LAYERS[layer]
    x = silu_inputs(layer, T, name)[0]
    wg, wu, wd = what(layer, "silu", stored)
    if exchanged:
        wg, wu = wu, wg
    zero = np.zeros(hidden)
    d, e_d = np.zeros((T, count, k_out)), np.zeros((T, count, k_out))
    for e in range(count):
        h64, b_h = _silu_bound(x, wg[e], zero, wu[e], zero)
        assert np.array_equal(h64, _silu64(x.astype(np.float64) @ wg[e].T) * (x.astype(np.float64) @ wu[e].T))
        hb, e_h = _store_bf16(h64, b_h)
        d[:, e] = hb @ wd[e].T
        e_d[:, e] = e_h @ np.abs(wd[e]).T + (hidden + 2) * U24 * (np.abs(hb) @ np.abs(wd[e]).T)
    return _frozen(d), _frozen(e_d)


def silu_want(layer, stored, T, name, ids, w, base, expert_dtype, out_dtype, exchanged=False):
    """(y float64 (T, k_out) as out_dtype holds it, E_y) for GIVEN ids and weights (T, K) and base (None or (T, k_out))."""
    d, e_d = silu_rows(layer, stored, T, name, exchanged)
    if expert_dtype == "bfloat16":
        d, e_d = _store_bf16(d, e_d)
    ids, w = np.asarray(ids), np.asarray(w, dtype=np.float32)
    y, mass = _combine64(d, ids, w, base)
    e_y = _combine64(e_d, ids, np.abs(w), None)[0] + (ids.shape[1] + 2) * U24 * mass
    if out_dtype == "bfloat16":
        y, e_y = _store_bf16(y, e_y)
    return y, e_y


def check_exchange_is_seen(layer, stored, T, name, ids, w, base, expert_dtype, out_dtype):
    """The condition: with gate and up exchanged the reference leaves the bound on some output of every token with a live slot."""
    y, e_y = silu_want(layer, stored, T, name, ids, w, base, expert_dtype, out_dtype)
    other, _e = silu_want(layer, stored, T, name, ids, w, base, expert_dtype, out_dtype, exchanged=True)
    ids = np.asarray(ids)
    live = ((ids >= 0) & (ids < LAYERS[layer][0])).any(axis=1)
    seen = (np.abs(other - y) > e_y).any(axis=1)
    assert live.any() and seen[live].all(), (layer, stored, T, name, np.flatnonzero(live & ~seen)[:8])


# ----------------------------------------------------------------------------- the expert modules alone

def rows_of_plan(ids, count):
    """(group_rows, R, the token of every expert row, the expert of every expert row) of the contract's plan."""
    group_rows, _row_of, src = _want_plan(np.asarray(ids), count)
    R = int(group_rows[-1])
    return group_rows, R, src[:R].astype(np.int64) // np.asarray(ids).shape[1], np.repeat(np.arange(count), np.diff(group_rows))


@functools.lru_cache(maxsize=None)
def dense_experts(layer, tier, stored, backend="emulation"):
    """(gate, up, down) of expert DENSE_EXPERT packed on its own: pack of W for "rows", pack_transposed of W for "transpose"."""
    pack = packed.pack if stored == "rows" else packed.pack_transposed
    return tuple(pack(np.array(w[DENSE_EXPERT]), m[DENSE_EXPERT], backend=backend) for w, m in zip(weights(layer, tier), maps(layer, stored)))
