"""The MoE router cases that tests/test_packed_moe_route_gpu.py (the kernels of csrc/mtq_moe_route.hip) and
tests/test_packed_moe_route_host.py (the emulation) both draw: the shapes, the inputs, and the want-side in two independent pieces,
neither of them the code under test.  NumPy only: no fixture, no device.

  want_select   the contract's rule (include/mtq.h "MoE router") on GIVEN float32 scores, token by token in plain NumPy float32: key,
                ranking, groups, ids and weights, each operation rounded once.  Holds for every token of every case, ties and special
                values included: the ids and weight words under test must equal want_select of the scores under test.
  reference64   the same routing in float64 from the logits, with the smallest relative gap, per token, over the comparisons the
                result depends on: adjacent keys from rank 1 to rank K + 1 among the remaining experts, adjacent group scores from
                rank 1 to topk_group + 1.  The ids under test must equal its ids on the tokens whose gap is at least GAP, and at
                least QUALIFY of a case's tokens must be such tokens (asserted on the want-side, before the code under test is asked).

The generator: each row a random permutation of (e - count // 2) * 8 / max(count, 8) in float32, so |logit| <= 4 and
|logit - row max| <= 8 = SPREAD; a bias of multiples of 1/256 in [0, 0.25).  The score bound on those inputs, relative to float64:
(2 * ceil(SPREAD * log2 e) + ceil(log2 count) + 8) * 2^-24: the half-ulp roundings of the shifted argument and of its scaling to base
2, amplified by the exponent; a lane-then-butterfly sum of positive terms; the ulps of exp2, the add, the divide and the per-lane
partial sums.

The launch geometry of csrc/mtq_moe_route.hip's host code is written out once more (route_path, route_grid), so that a test can state
in code which kernel and which trip of the token loop its shape meets.
"""
from __future__ import annotations

import functools
import math

import numpy as np

SENTINEL = 0xA5
GAP = 2.0 ** -15                # the ids are compared with reference64's where the decisive comparisons are at least this far apart
QUALIFY = 0.9                   # and at least this share of a case's tokens must be such tokens
SPREAD = 8.0

# (count, topk, tokens): tokens from {1, 3, 5, 67}, so that a workgroup's last wave is ragged
UNGROUPED = ((1, 1, 5), (2, 1, 3), (8, 2, 67), (8, 8, 1), (60, 5, 67), (64, 6, 67), (65, 3, 67), (128, 8, 67), (129, 8, 5), (256, 8, 67),
             (257, 8, 67), (384, 8, 67), (4096, 64, 3))
# (count, topk, n_group, topk_group, group_top, tokens)
GROUPED = ((256, 8, 8, 4, 2, 67), (160, 6, 8, 3, 1, 67), (320, 8, 64, 8, 2, 67), (64, 4, 64, 4, 1, 67), (32, 8, 4, 2, 2, 67),
           (256, 8, 8, 8, 2, 67),
           # n_group no power of two: kept_groups gives group g the lanes g << per_log2 of P = the power of two at or above n_group, so
           # the lanes of groups n_group .. P - 1 are idle and must stay out of the ballot and the butterfly
           (96, 4, 3, 2, 2, 67),                          # two experts a lane; 16 idle lanes
           (60, 6, 6, 3, 1, 67),                          # one expert a lane; groups of 10; 16 idle lanes
           (240, 8, 12, 5, 2, 67),                        # four experts a lane
           (384, 8, 24, 6, 2, 67),                        # the LDS kernel; two lanes a group
           (120, 6, 5, 2, 2, 67),                         # groups of 24; 24 idle lanes
           (330, 8, 33, 8, 1, 5),                         # the LDS kernel; a lane a group; 31 idle lanes
           (192, 8, 48, 12, 1, 67))
# (score, with a bias, renormalize, eps, scale): both scores with and without a bias, both renormalize, both eps, both scales
VARIANTS = (("softmax", False, True, 0.0, 1.0), ("softmax", True, False, 0.0, 2.5), ("sigmoid", False, False, 1e-20, 1.0),
            ("sigmoid", True, True, 1e-20, 2.5), ("softmax", True, True, 1e-20, 2.5), ("sigmoid", False, True, 0.0, 1.0))

# csrc/mtq_moe_route.hip: kRouteRegWaves, kRouteRegMaxCount, kRouteMaxBlocks
REG_WAVES, REG_MAX_COUNT, MAX_BLOCKS = 4, 256, 2048


def route_path(count: int):
    """(experts a lane holds in registers, or 0 for the LDS kernel; tokens a workgroup), as the host code picks them."""
    per = 1 if count <= 64 else 2 if count <= 128 else 4 if count <= REG_MAX_COUNT else 0
    return per, (REG_WAVES if per else 1)


def route_grid(tokens: int, count: int):
    """(workgroups, trips of workgroup 0 through the token loop)."""
    _per, waves = route_path(count)
    blocks = min(-(-tokens // waves), MAX_BLOCKS)
    return blocks, -(-tokens // (blocks * waves))


def score_bound(count: int) -> float:
    return (2 * math.ceil(SPREAD * math.log2(math.e)) + math.ceil(math.log2(count)) + 8) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def logits_of(tokens: int, count: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(100003 * count + 17 * tokens + seed)
    base = ((np.arange(count) - count // 2) * (8.0 / max(count, 8))).astype(np.float32)
    x = np.stack([base[rng.permutation(count)] for _ in range(tokens)])
    assert x.dtype == np.float32 and np.abs(x).max() <= 4 and (x.max(axis=1, keepdims=True) - x).max() <= SPREAD
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def bias_of(count: int, seed: int = 0, negative: bool = False) -> np.ndarray:
    rng = np.random.default_rng(7919 * count + seed)
    b = (rng.integers(0, 64, size=count) / 256.0).astype(np.float32)
    if negative:
        b = (b - np.float32(0.125)).astype(np.float32)
        assert (b < 0).any() or count < 4
    b.setflags(write=False)
    return b


# ----------------------------------------------------------------------------- the rule on given float32 scores

def _rank_value(v):
    """A key as the ranking sees it: NaN as -Inf, -0 as +0 (float32 or float64 alike)."""
    if np.isnan(v):
        return type(v)(-np.inf)
    return v + type(v)(0)


def _ranked(keys, ids):
    """ids sorted by the contract: key descending, ties to the lower id."""
    return sorted(ids, key=lambda e: (-float(keys[e]), e))


def _route_token(keys, topk, n_group, topk_group, group_top):
    """The selection of one token on its ranking keys (a list of NumPy scalars of one type) → (ids in rank order, remaining experts in
    rank order, group scores in rank order or None)."""
    count = len(keys)
    remaining = list(range(count))
    group_scores = None
    if n_group > 1:
        size = count // n_group
        scores = []
        for g in range(n_group):
            inside = _ranked(keys, range(g * size, (g + 1) * size))
            s = keys[inside[0]]
            if group_top == 2:
                s = s + keys[inside[1]]                    # one rounding in the keys' type
            scores.append(_rank_value(s))
        order = _ranked(scores, range(n_group))
        kept = set(order[:topk_group])
        remaining = [e for e in remaining if e // size in kept]
        group_scores = [scores[g] for g in order]
    ranked = _ranked(keys, remaining)
    return ranked[:topk], ranked, group_scores


def want_select(scores32, bias, topk, n_group=1, topk_group=1, group_top=2, renormalize=True, eps=0.0, scale=1.0):
    """(ids int32 (T, topk), weights float32 (T, topk)) by the contract on float32 scores (T, count): every operation a NumPy float32
    scalar operation, rounded once."""
    scores32 = np.asarray(scores32)
    assert scores32.dtype == np.float32 and scores32.ndim == 2
    T, count = scores32.shape
    eps32, scale32 = np.float32(eps), np.float32(scale)
    ids = np.zeros((T, topk), dtype=np.int32)
    weights = np.zeros((T, topk), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(T):
            s = scores32[t]
            keys = [_rank_value(s[e] if bias is None else s[e] + np.float32(bias[e])) for e in range(count)]
            assert all(type(k) is np.float32 for k in keys)
            chosen, _ranked_all, _groups = _route_token(keys, topk, n_group, topk_group, group_top)
            v = [s[e] for e in chosen]
            if renormalize:
                d = v[0]
                for j in range(1, topk):
                    d = d + v[j]
                d = d + eps32
                w = [(x / d) * scale32 for x in v]
            else:
                w = [x * scale32 for x in v]
            assert all(type(x) is np.float32 for x in w)
            ids[t], weights[t] = chosen, w
    return ids, weights


# ----------------------------------------------------------------------------- the routing in float64 from the logits

def _gap(a: float, b: float) -> float:
    if a == b:
        return 0.0
    if np.isinf(a) or np.isinf(b):
        return np.inf
    return float((a - b) / max(abs(a), abs(b)))


def scores64(logits, score: str) -> np.ndarray:
    x = np.asarray(logits, dtype=np.float64)
    if score == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    p = np.exp(x - x.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def reference64(logits, score, bias, topk, n_group=1, topk_group=1, group_top=2):
    """(ids (T, topk), scores float64 (T, count), gap float64 (T,)) from finite logits."""
    s = scores64(logits, score)
    T, count = s.shape
    ids = np.zeros((T, topk), dtype=np.int32)
    gap = np.zeros(T, dtype=np.float64)
    for t in range(T):
        keys = [np.float64(s[t, e]) + (np.float64(0) if bias is None else np.float64(bias[e])) for e in range(count)]
        chosen, ranked, groups = _route_token(keys, topk, n_group, topk_group, group_top)
        gaps = [_gap(float(keys[a]), float(keys[b])) for a, b in zip(ranked[:topk], ranked[1: topk + 1])]
        if groups is not None:
            gaps += [_gap(float(a), float(b)) for a, b in zip(groups[:topk_group], groups[1: topk_group + 1])]
        ids[t], gap[t] = chosen, min(gaps, default=np.inf)
    return ids, s, gap


def ids_comparable(count: int, variant) -> bool:
    """Whether a case's ids go to reference64.  Not softmax with a bias from 256 experts on: the scores there are about 1 / count and
    less, the bias is multiples of 1/256 up to 0.25, so the experts of the best bias value are ranked by score differences of
    1e-6 of the key and less than 90 % of the tokens have clear comparisons (82 % at 256, 88 % at 384 in float64).  Those cases keep
    want_select on every token and the score bound; the routers that carry a bias score with sigmoid."""
    score, with_bias = variant[0], variant[1]
    return not (score == "softmax" and with_bias and count >= 256)


def check_against_reference64(got_ids, got_scores, logits, score, bias, topk, n_group=1, topk_group=1, group_top=2, what="", compare_ids=True):
    """The independent checks on the generator's inputs: the condition on the want-side first (enough tokens with clear comparisons),
    then the ids on those tokens and the score error on all.  Returns the largest relative score error."""
    want_ids, s64, gap = reference64(logits, score, bias, topk, n_group, topk_group, group_top)
    if compare_ids:
        clear = gap >= GAP
        assert clear.mean() >= QUALIFY, (what, float(clear.mean()))
        assert np.array_equal(np.asarray(got_ids)[clear], want_ids[clear]), (what, np.flatnonzero((np.asarray(got_ids) != want_ids).any(axis=1) & clear)[:8])
    err = float(np.max(np.abs(np.asarray(got_scores, dtype=np.float64) - s64) / s64))
    return err


def ungrouped_cases():
    for i, (count, topk, tokens) in enumerate(UNGROUPED):
        yield count, topk, 1, 1, min(2, count), tokens, VARIANTS[i % len(VARIANTS)]      # group_top <= count / n_group at every n_group


def grouped_cases():
    for i, (count, topk, n_group, topk_group, group_top, tokens) in enumerate(GROUPED):
        yield count, topk, n_group, topk_group, group_top, tokens, VARIANTS[(i + 3) % len(VARIANTS)]
