"""Layer-output error (csrc/mtq_output_error.hip) on inputs where the kernel's f32 arithmetic is exact.

On such inputs every output the kernel forms equals the float64 emulation's output, so its sums may differ from
`emulation_sums` only by the order of the float64 additions, with no ε term: one wrong product in one candidate image shows.
  * integer grid — X integers |x| ≤ 4 (bf16), W and the bias on the 2⁻⁸ grid with |w| < 1: every BFP image stays on the grid and
    every partial sum below 2²⁴ grid units, so X·Ŵᵀ is exact in any order; where a float64 sum of grid values is exact too,
    the kernel's sum must equal the emulation's;
  * one-hot — each row of X holds one 2ˢ, so each output is 2ˢ times one element of W or Ŵ: exact for a full 24-bit mantissa,
    which pins the in-LDS quantiser and the three-way split hi + mid + lo = W of float32 weights.
The preconditions are asserted on the host for every case (the host tests below run them without a GPU), and the comparison
returns a verdict so that the tests can show they fail on a wrong image."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import SLOTS, emulation_sums, hip_sums
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen, to_bf16_valued

FMTS = ["bf16", "bfp8", "bfp4", "bfp2"]
GRID = 2.0 ** -8
TILE = 32
F64 = 2.0 ** -53
NORMAL = 2.0 ** -126
gpu = pytest.mark.gpu


# ----------------------------------------------------------------------------- oracle, bounds and the verdict


def formats_of(mask: int) -> list:
    return [f for i, f in enumerate(FMTS) if mask >> i & 1]


def slots_of(mask: int, with_map: bool, with_rec: bool) -> list:
    """The slots a launch writes: the requested formats, the map, fp0 (always) and the recorded output."""
    return [i for i in range(4) if mask >> i & 1] + ([4] if with_map else []) + [5] + ([6] if with_rec else [])


def map_image(w32: np.ndarray, amap: np.ndarray, images=None) -> np.ndarray:
    """The map candidate's Ŵ built tile by tile on the host: each 32 × 32 tile of W quantised by its code with
    quantize_weight_values (or taken from `images[fmt]`, e.g. the reference's own bits).  No GPU kernel is involved."""
    y = np.zeros_like(w32)
    for ti in range(amap.shape[0]):
        for tj in range(amap.shape[1]):
            sl = np.s_[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
            f = FMTS[int(amap[ti, tj])]
            y[sl] = quantize_weight_values(w32[sl], f) if images is None else images[f][sl]
    return y


def bounds(r, q, unit=None, dr=0.0, dq=0.0):
    """What the kernel's seven sums of one slot may differ from the emulation's by, given the exact per-output values r, q.
    → (exact[7], tol[7]).  Without a split residual (dr = dq = 0) max|r − q| is exact; Σr, Σr², Σq, Σq², Σrq and Σ|r − q| are exact
    when every term is a multiple of `unit` (unit² for the products) and Σ|term| stays below 2⁵³ units, which makes any float64
    summation order exact; otherwise they may differ by 64·MN·2⁻⁵³·Σ|term|.  dr, dq: per-output bounds of |Δr|, |Δq| (the split
    residual of weights below 2⁻¹⁰⁰), added to the tolerance by first-order propagation."""
    r, q = np.asarray(r, np.float64).ravel(), np.asarray(q, np.float64).ravel()
    dr, dq = np.broadcast_to(np.asarray(dr, np.float64).ravel(), r.shape), np.broadcast_to(np.asarray(dq, np.float64).ravel(), r.shape)
    ar, aq = np.abs(r), np.abs(q)
    mags = np.array([ar.sum(), (ar * ar).sum(), aq.sum(), (aq * aq).sum(), (ar * aq).sum(), np.abs(r - q).sum(), 0.0])
    split = np.zeros(7)
    if dr.any() or dq.any():
        split = np.array([dr.sum(), (2 * ar * dr + dr * dr).sum(), dq.sum(), (2 * aq * dq + dq * dq).sum(),
                          (ar * dq + aq * dr + dr * dq).sum(), (dr + dq).sum(), (dr + dq).max(initial=0.0)])
    tol = 64 * r.size * F64 * mags + split
    exact = split == 0.0
    for j, p in enumerate((1, 2, 1, 2, 2, 1)):
        exact[j] &= unit is not None and mags[j] < 2.0 ** 53 * unit ** p
    return exact, tol


def verdict(got, want, expect: dict) -> list:
    """Compare two [7, 7] sums → a list of mismatches (empty: they agree).  expect: slot → (exact[7], tol[7]); every other slot
    must be zero in both.  Non-finite values agree only with the same value (NaN with NaN)."""
    bad = []
    for s in range(len(SLOTS)):
        exact, tol = expect.get(s, (np.ones(7, bool), np.zeros(7)))
        for j in range(7):
            g, w = float(got[s][j]), float(want[s][j])
            if not (np.isfinite(g) and np.isfinite(w)):
                ok = g == w or (np.isnan(g) and np.isnan(w))
            elif exact[j]:
                ok = g == w
            else:
                ok = abs(g - w) <= tol[j]
            if not ok:
                bad.append((SLOTS[s], j, g, w, "exact" if exact[j] else float(tol[j])))
    return bad


# ----------------------------------------------------------------------------- integer-grid cases


def grid_operands(m, n, k, seed, with_bias):
    """X integers in [-4, 4]; W on the 2⁻⁸ grid, |w| ≤ 255/256, each 16-group drawn at one of four magnitudes (shared exponents
    and BFP steps differ from group to group; odd grid values are exact BFP ties); the bias on the same grid."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(m, k)).astype(np.float32)
    lim = np.repeat(rng.choice([255, 63, 7, 1], size=(n, -(-k // 16))), 16, axis=1)[:, :k]
    w = (rng.integers(-lim, lim + 1) * GRID).astype(np.float32)
    bias = (rng.integers(-255, 256, size=n) * GRID).astype(np.float32) if with_bias else None
    return x, w, bias


def assert_grid_exact(x, images, bias) -> None:
    """The precondition of the exact comparison, checked rather than assumed: X holds integers |x| ≤ 4 (exact in bf16); every
    image the kernel multiplies (W and each candidate's Ŵ, from the oracle) and the bias lie on the 2⁻⁸ grid with |v| ≤ 1; and the
    worst-case |partial sum| of any output, 4·max_n Σ_k |v_nk| + max|b|, stays below 2²⁴ grid units.  Then every f32 partial sum
    the kernel forms is exact in any order, and so are R and every Y."""
    assert np.array_equal(x, np.round(x)) and np.abs(x).max(initial=0) <= 4
    b = np.zeros(1) if bias is None else np.asarray(bias, np.float64)
    for v in [*images, b]:
        u = np.asarray(v, np.float64) / GRID
        assert np.array_equal(u, np.round(u)) and np.abs(v).max(initial=0) <= 1.0
    worst = max(4 * np.abs(np.asarray(v, np.float64)).sum(axis=1).max(initial=0) for v in images) + np.abs(b).max()
    assert worst / GRID < 2.0 ** 24, worst


def grid_expect(x, w, bias, images: dict, rec, with_map: bool, mask: int) -> dict:
    """slot → bounds() of a grid case from the exact per-output values (images: format → Ŵ, plus "map")."""
    x64 = np.asarray(x, np.float64)
    b = 0.0 if bias is None else np.asarray(bias, np.float64)
    r = x64 @ np.asarray(w, np.float64).T + b
    out = {}
    for s in slots_of(mask, with_map, rec is not None):
        if s < 5:
            q = x64 @ np.asarray(images[SLOTS[s]], np.float64).T + b
        elif s == 5:
            q = np.broadcast_to(b, r.shape)
        else:
            q = np.asarray(rec, np.float64)
        out[s] = bounds(r, q, unit=GRID)
    return out


MS = (1, 127, 128, 129, 300)
NS = (1, 63, 64, 65, 130, 576)
KS = (1, 15, 16, 17, 33, 64, 65, 200, 7171)
BIG_K = {(1, 1), (127, 130), (129, 65), (300, 576)}     # the K = 7171 shapes: single output and multi-block ragged corners


def sweep_cases(k: int, with_bias: bool) -> list:
    """(m, n, k, seed, fmt_mask, bf16 storage, with map, with recorded) of one K: the full M × N cross product for K < 7171, the
    ragged corners for K = 7171, and a kv_a_proj-like shape (N = 576, K = 7168) next to it.  fmt_mask walks 1..15, the storage
    alternates (15 and 2 are coprime, so every mask meets both), every fourth case adds a random map, every third a recorded output."""
    shapes = [(m, n, k) for m in MS for n in NS if k != 7171 or (m, n) in BIG_K] + ([(300, 576, 7168)] if k == 7171 else [])
    base = KS.index(k) * 64 + 1000 * with_bias
    return [(m, n, kk, base + i, 1 + (base + i) % 15, (base + i) % 2 == 1, (base + i) % 4 == 1, (base + i) % 3 == 0)
            for i, (m, n, kk) in enumerate(shapes)]


def grid_case(m, n, k, seed, mask, bf16w, with_map, with_rec, with_bias):
    """A sweep case's operands, oracle images and expectation; asserts the precondition."""
    x, w, bias = grid_operands(m, n, k, seed, with_bias)
    images = {f: quantize_weight_values(w, f) for f in formats_of(mask)}
    amap = None
    if with_map:
        th, tw = hb.tiles_hw(n, k)
        amap = np.random.default_rng(seed + 7).integers(0, 4, size=(th, tw)).astype(np.int8)
        images["map"] = map_image(w, amap)
    assert_grid_exact(x, [w, *images.values()], bias)
    rec = None
    if with_rec:   # bf16 storage of R: coarser steps, still on the grid
        rec = to_bf16_valued(np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + (0.0 if bias is None else bias))
    return x, w, bias, amap, images, rec


def run_both(x, w, bias, mask, amap, images, rec, bf16w, chunk_rows=None):
    """(kernel sums, emulation sums) of one case; the map oracle goes to the emulation as map_y."""
    xt = torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16)
    wt = torch.from_numpy(w).to(torch.bfloat16 if bf16w else torch.float32)
    bt = None if bias is None else torch.from_numpy(bias)
    rt = None if rec is None else torch.from_numpy(np.asarray(rec, np.float32))
    step = chunk_rows or xt.shape[0]
    chunks = lambda: [Chunk(x=xt[s: s + step], recorded=None if rt is None else rt[s: s + step]) for s in range(0, xt.shape[0], step)]
    got, *_ = hip_sums(chunks(), wt, formats_of(mask), bt, amap)
    want, *_ = emulation_sums(chunks(), wt, formats_of(mask), bt, None if amap is None else images["map"])
    return got, want


# ----------------------------------------------------------------------------- one-hot cases


def split3(w32: np.ndarray):
    """The kernel's reference split of float32 W: hi = bf16(W), mid = bf16(W − hi), lo = bf16(W − hi − mid)."""
    hi = to_bf16_valued(w32)
    d1 = (w32 - hi).astype(np.float32)
    mid = to_bf16_valued(d1)
    return hi, mid, to_bf16_valued((d1 - mid).astype(np.float32))


def _groups(a: np.ndarray) -> np.ndarray:
    n, k = a.shape
    return np.pad(np.abs(a.astype(np.float64)), ((0, 0), (0, -k % 16))).reshape(n, -1, 16)


def onehot_launches(w32: np.ndarray, images: dict) -> list:
    """Partition W's 16-groups into launches of one power-of-two scale s each → [(group mask (n, k/16), s, tiny)].

    Every value the kernel multiplies (hi, mid, lo and each Ŵ) must give a normal f32 product 2ˢ·v and be a normal bf16, so a
    launch spans at most 2²⁵⁰ from its smallest non-zero value to its largest; and its group maxima span at most 2⁸, so that one
    bfp8 step of its smallest group still moves Σq past the float64 tolerance of the whole launch (asserted in onehot_case).
    Groups whose largest |W| is below 2⁻¹⁰⁰, or that hold a part below the normal range, go into one launch of their own (`tiny`),
    where the split may lose its subnormal parts."""
    parts = [_groups(v) for v in (*split3(w32), *images.values())]
    vmax = np.max([p.max(axis=2) for p in parts], axis=0)
    vmin = np.min([np.where(p > 0, p, np.inf).min(axis=2) for p in parts], axis=0)
    sub = np.any([((p > 0) & (p < NORMAL)).any(axis=2) for p in parts], axis=0)
    live = vmax > 0
    tiny = live & ((_groups(w32).max(axis=2) < 2.0 ** -100) | sub)
    gmax = _groups(w32).max(axis=2)
    out = []
    rest = np.argwhere(live & ~tiny)
    order = rest[np.argsort(gmax[tuple(rest.T)], kind="stable")]
    while len(order):
        lo, hi, g = vmin[tuple(order.T)], vmax[tuple(order.T)], gmax[tuple(order.T)]
        fits = (np.maximum.accumulate(hi) / np.minimum.accumulate(lo) < 2.0 ** 250) & (g <= g[0] * 2.0 ** 8)
        take = max(1, int(np.argmin(fits)) if not fits.all() else len(order))
        gm = np.zeros(vmax.shape, bool)
        gm[tuple(order[:take].T)] = True
        out.append((gm, _scale(vmax[gm].max()), False))
        order = order[take:]
    if tiny.any():
        out.append((tiny, _scale(vmax[tiny].max()), True))
    return out


def _scale(vmax: float) -> int:
    return int(min(127, 125 - np.floor(np.log2(vmax))))


def onehot_case(w32, images, gmask, s, tiny, seed):
    """One launch: W and the images restricted to the groups of gmask, X = 2ˢ·P (P a random K × K permutation), the exact
    outputs r = 2ˢ·W[:, perm]ᵀ, q_f = 2ˢ·Ŵ_f[:, perm]ᵀ, and the expectation (with the split residual of a tiny launch)."""
    n, k = w32.shape
    keep = np.repeat(gmask, 16, axis=1)[:, :k]
    wc = np.where(keep, w32, np.float32(0)).astype(np.float32)
    imc = {f: np.where(keep, v, np.float32(0)).astype(np.float32) for f, v in images.items()}
    parts = [*split3(wc), *imc.values()]
    scale = 2.0 ** s
    nz = np.concatenate([np.abs(p[p != 0]).astype(np.float64) for p in parts])
    if not tiny:   # the precondition: every part a normal bf16 and every product 2ˢ·v a normal, finite f32
        assert nz.size == 0 or (nz.min() >= NORMAL and nz.min() * scale >= NORMAL and nz.max() * scale < 2.0 ** 127), (s, nz.min(), nz.max())
    else:
        assert nz.max() * scale < 2.0 ** 127 and nz[nz >= NORMAL].min(initial=np.inf) * scale >= NORMAL
    perm = np.random.default_rng(seed).permutation(k)
    x = np.zeros((k, k), np.float32)
    x[np.arange(k), perm] = np.float32(scale)
    r = scale * wc.astype(np.float64)[:, perm].T
    hi = split3(wc)[0].astype(np.float64)
    dr = 0.0
    if tiny:   # the kernel's R may lose bf16-subnormal parts of the split: |Δ| ≤ 2ˢ·(3·|W − hi| + |hi| if hi is subnormal)
        dr = scale * (3 * np.abs(wc - hi) + np.where(np.abs(hi) < NORMAL, np.abs(hi), 0.0))[:, perm].T
    expect = {}
    for slot, key in enumerate(SLOTS[:5]):
        if key in imc:
            qv = imc[key].astype(np.float64)
            dq = scale * np.where(np.abs(qv) < NORMAL, np.abs(qv), 0.0)[:, perm].T if tiny else 0.0
            expect[slot] = bounds(r, scale * qv[:, perm].T, None, dr, dq)
    expect[5] = bounds(r, np.zeros_like(r), None, dr, 0.0)
    if not tiny:   # sensitivity: one bfp8 step of any live group (2^(e − 6), e its shared exponent) moves Σq past the tolerance
        gm = _groups(wc).max(axis=2)
        step = scale * 2.0 ** (np.floor(np.log2(gm[gm > 0].min())) - 6)
        for slot in {SLOTS.index(f) for f in ("bfp8", "map")} & set(expect):
            assert step > expect[slot][1][2], (slot, step, expect[slot][1][2])
    return x, wc, imc, expect


def edge_weights() -> np.ndarray:
    """Heavy-tailed float32 W (ragged: 70 × 200) with planted groups: shared exponents 79, 80, 180 and 181 (the borders of the
    quantiser's exact route), one value per two binades, 1.9999999 (saturating round-up in every format), exact ties, a row near
    2⁹⁰, groups below 2⁻¹⁰⁰ and an all-zero group."""
    rng = np.random.default_rng(31)
    w = gen("heavy_f32", 17, (70, 200)).copy()
    for r, e in ((9, 79), (10, 80), (11, 180), (12, 181)):
        w[r, 48:64] = (1.0 + rng.random(16)).astype(np.float32) * np.float32(2.0 ** (e - 127)) * np.where(rng.random(16) < 0.5, -1, 1)
    w[13, 64:80] = np.ldexp(np.float32(1.0), -np.arange(16, dtype=np.int32) * 2).astype(np.float32)
    w[14, 64:80] = np.float32(1.9999999)
    ties = [k * 2.0 ** (1 - m) + 2.0 ** -m for m in (7, 3, 1) for k in range(4) if k * 2.0 ** (1 - m) + 2.0 ** -m < 2]
    w[15, 0:16] = np.array([1.0] + ties + [-1.5, 0.0, -0.625, 1.75, 0.25], dtype=np.float32)   # exact ties, group maximum in [1, 2)
    w[16, :] *= np.float32(2.0 ** 90)
    w[17, 16:48] = (rng.standard_normal(32) * 2.0 ** -105).astype(np.float32)
    w[18, 32:48] = 0.0
    w[19, 192:200] = (rng.standard_normal(8) * 2.0 ** -110).astype(np.float32)     # the padded last group of a row, tiny
    return w


def f1_weights(golden_dir):
    """The F1 known-answer vectors as W rows, groups holding Inf/NaN zeroed in W and in the reference's own images."""
    d = np.load(golden_dir / "f1_quantize_kat.npz")
    w = d["x_bits"].view(np.float32).copy()
    bad = np.repeat(~np.isfinite(w).reshape(w.shape[0], -1, 16).all(axis=2), 16, axis=1)
    w[bad] = 0.0
    images = {f: np.where(bad, np.float32(0), d[f"y_{f}"].view(np.float32)).astype(np.float32) for f in FMTS}
    return w, images


# ----------------------------------------------------------------------------- host tests (no GPU)


def test_grid_precondition_holds_for_every_sweep_case():
    masks = set()
    for k in KS:
        for with_bias in (False, True):
            for (m, n, kk, seed, mask, bf16w, with_map, with_rec) in sweep_cases(k, with_bias):
                grid_case(m, n, kk, seed, mask, bf16w, with_map, with_rec, with_bias)
                masks.add((mask, bf16w))
    assert masks == {(mk, b) for mk in range(1, 16) for b in (False, True)}


def test_onehot_launch_preconditions(golden_dir):
    """The one-hot partitions cover every live group once and meet their precondition; the F1 images are quantize_weight_values'."""
    w = edge_weights()
    images = {f: quantize_weight_values(w, f) for f in FMTS}
    launches = onehot_launches(w, images)
    assert sum(gm.astype(int) for gm, _, _ in launches).max() == 1 and sum(t for *_, t in launches) == 1 and len(launches) >= 2
    for i, (gm, s, tiny) in enumerate(launches):
        onehot_case(w, images, gm, s, tiny, i)
    wf, gold = f1_weights(golden_dir)
    for f in FMTS:
        assert np.array_equal(quantize_weight_values(wf, f).view(np.uint32), gold[f].view(np.uint32)), f
    for i, (gm, s, tiny) in enumerate(onehot_launches(wf, gold)):
        onehot_case(wf, gold, gm, s, tiny, i)


def test_verdict_sees_one_bfp_step():
    """Mutation check on the host: one element of the map's oracle image moved by one BFP step takes the emulation's sums out of
    what the exact comparison accepts; the unmoved image is accepted."""
    m, n, k = 129, 65, 70
    x, w, bias, amap, images, rec = grid_case(m, n, k, 5, 0xF, False, True, False, True)
    amap[-1, -1] = 2                                            # a bfp4 tile in the ragged corner
    images["map"] = map_image(w, amap)
    expect = grid_expect(x, w, bias, images, None, True, 0xF)
    xt, wt, bt = torch.from_numpy(x).to(torch.bfloat16), torch.from_numpy(w), torch.from_numpy(bias)
    base, *_ = emulation_sums([Chunk(x=xt)], wt, FMTS, bt, images["map"])
    assert verdict(base, base, expect) == []
    yb = images["map"].copy()
    i, j = n - 1, k - 1
    e = np.floor(np.log2(np.abs(w[i, (j // 16) * 16: j + 1]).max()))
    yb[i, j] += np.float32(2.0 ** (e - 2))                     # one bfp4 step of that group
    moved, *_ = emulation_sums([Chunk(x=xt)], wt, FMTS, bt, yb)
    bad = verdict(moved, base, expect)
    assert bad and {b[0] for b in bad} == {"map"}, bad


@pytest.mark.parametrize("where", ["first", "later"])
def test_emulation_atol_propagates_nan(where):
    """np.max semantics across M-chunks: a NaN recorded output makes the recorded row's atol NaN whichever chunk holds it."""
    w = np.array([[1.0, 0.0], [0.0, 1.0]], np.float32)
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]).to(torch.bfloat16)
    rec = x.float().clone()
    rec[0 if where == "first" else 2, 1] = float("nan")
    rec[1, 0] += 0.5
    sums, *_ = emulation_sums([Chunk(x=x[:1], recorded=rec[:1]), Chunk(x=x[1:], recorded=rec[1:])], w, ["bf16"])
    assert np.isnan(sums[SLOTS.index("recorded")][6]) and np.isnan(sums[SLOTS.index("recorded")][5])
    assert sums[SLOTS.index("bf16")][6] == 0.0
    # one chunk with r = [1, 2] against q = [NaN, 1.5]
    one, *_ = emulation_sums([Chunk(x=torch.tensor([[1.0, 2.0]]).to(torch.bfloat16), recorded=torch.tensor([[float("nan"), 1.5]]))], w, [])
    assert np.isnan(one[SLOTS.index("recorded")][6])
    # an Inf weight: R = Y = Inf for bf16, and ∞ − ∞ = NaN
    wi = np.array([[np.inf, 1.0], [0.5, 1.0]], np.float32)
    s2, *_ = emulation_sums([Chunk(x=torch.tensor([[1.0, 1.0]]).to(torch.bfloat16))], wi, ["bf16"])
    assert np.isnan(s2[SLOTS.index("bf16")][6])


# ----------------------------------------------------------------------------- GPU tests


@gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("k", KS)
def test_grid_sweep_exact(k, with_bias):
    """Every M × N of the sweep at this K: the kernel's sums against the emulation's, exactly where the float64 sums are exact."""
    torch.cuda.set_device(0)
    fails = []
    for (m, n, kk, seed, mask, bf16w, with_map, with_rec) in sweep_cases(k, with_bias):
        x, w, bias, amap, images, rec = grid_case(m, n, kk, seed, mask, bf16w, with_map, with_rec, with_bias)
        got, want = run_both(x, w, bias, mask, amap, images, rec, bf16w)
        bad = verdict(got, want, grid_expect(x, w, bias, images, rec, with_map, mask))
        if bad:
            fails.append(((m, n, kk, mask, "bf16" if bf16w else "f32", with_map, with_rec), bad[:4]))
    assert not fails, fails[:5]


MAP_SHAPES = [(129, 65, 200), (300, 97, 161), (37, 130, 33), (1, 33, 95), (200, 576, 257)]


@gpu
@pytest.mark.parametrize("bf16w", [False, True])
@pytest.mark.parametrize("m,n,k", MAP_SHAPES)
def test_map_ragged_exact(m, n, k, bf16w):
    """Hand-made maps (a random code in every tile) on shapes ragged in N and K against the host's tile-by-tile oracle image."""
    torch.cuda.set_device(0)
    seed = m + 3 * n + 7 * k
    x, w, bias, amap, images, rec = grid_case(m, n, k, seed, 0xF, bf16w, True, False, True)
    assert set(np.unique(amap)) == {0, 1, 2, 3}
    got, want = run_both(x, w, bias, 0xF, amap, images, rec, bf16w)
    bad = verdict(got, want, grid_expect(x, w, bias, images, None, True, 0xF))
    assert not bad, bad


@gpu
def test_map_one_tile_mutation_is_reported():
    """The kernel run with a map that differs from the oracle's in the ragged corner tile: the verdict reports the map slot."""
    torch.cuda.set_device(0)
    m, n, k = 129, 65, 200
    x, w, bias, amap, images, rec = grid_case(m, n, k, 77, 0xF, False, True, False, True)
    expect = grid_expect(x, w, bias, images, None, True, 0xF)
    bad_map = amap.copy()
    bad_map[-1, -1] = (amap[-1, -1] + 2) % 4
    assert not np.array_equal(map_image(w, bad_map), images["map"])
    got, want = run_both(x, w, bias, 0xF, amap, images, None, False)
    assert verdict(got, want, expect) == []
    got_bad, _ = run_both(x, w, bias, 0xF, bad_map, images, None, False)
    bad = verdict(got_bad, want, expect)
    assert bad and {b[0] for b in bad} == {"map"}, bad


def _onehot_run(w, images, tile_images=None):
    """Every one-hot launch of W (float32 storage, all formats and a random map) → failures.  The map's oracle image is built
    tile by tile from quantize_weight_values, or from `tile_images` (format → image) when given."""
    fails = []
    th, tw = hb.tiles_hw(*w.shape)
    for i, (gm, s, tiny) in enumerate(onehot_launches(w, images)):
        amap = np.random.default_rng(200 + i).integers(0, 4, size=(th, tw)).astype(np.int8)
        x, wc, imc, expect = onehot_case(w, {**images, "map": map_image(w, amap, tile_images)}, gm, s, tiny, 100 + i)
        got, want = run_both(x, wc, None, 0xF, amap, imc, None, False)
        bad = verdict(got, want, expect)
        if bad:
            fails.append((i, s, tiny, bad[:4]))
    return fails


@gpu
def test_onehot_heavy_f32_and_edge_groups():
    """Heavy-tailed float32 W with edge groups: each output is one element of W or Ŵ, so hi + mid + lo = W and every quantised
    element (fast and literal route, ties, saturation) is pinned."""
    torch.cuda.set_device(0)
    w = edge_weights()
    fails = _onehot_run(w, {f: quantize_weight_values(w, f) for f in FMTS})
    assert not fails, fails


@gpu
def test_onehot_f1_known_answer_vectors(golden_dir):
    """The F1 vectors as W rows against the reference's own y_bfp* bits (for the pure formats and, tile by tile, for the map)."""
    torch.cuda.set_device(0)
    w, gold = f1_weights(golden_dir)
    fails = _onehot_run(w, gold, tile_images=gold)
    assert not fails, fails


def _sentinels() -> np.ndarray:
    s = np.array([[(1 + i + 0.125 * j) * (-1) ** j for j in range(7)] for i in range(len(SLOTS))], np.float64)
    s[:, 6] = [0.5, 1e6, 0.25, 1e6, 0.75, 1e6, 0.5]             # max: below and above the launch's max|r − q|
    return s


@gpu
def test_slot_isolation_and_accumulation():
    """sums pre-filled with sentinels, every mask with and without the map and the recorded output: unrequested slots keep their
    bits, requested ones become sentinel + (a launch from zero) bit for bit, their max fmax(sentinel, fresh)."""
    torch.cuda.set_device(0)
    m, n, k = 129, 65, 70
    x, w, bias, amap, images, rec = grid_case(m, n, k, 9, 0xF, False, True, True, True)
    xd = torch.from_numpy(x).to(torch.bfloat16).cuda()
    wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda()
    ad, rd = torch.from_numpy(amap).cuda(), torch.from_numpy(rec).to(torch.bfloat16).cuda()
    sent = _sentinels()
    fails = []
    for mask in range(1, 16):
        for use_map in (False, True):
            for use_rec in (False, True):
                args = dict(bias=bd, assignment=ad if use_map else None, recorded=rd if use_rec else None)
                fresh = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
                acc = torch.from_numpy(sent.copy()).cuda()
                hb.output_error(xd, wd, mask, fresh, **args)
                hb.output_error(xd, wd, mask, acc, **args)
                torch.cuda.synchronize()
                f, a = fresh.cpu().numpy(), acc.cpu().numpy()
                want = sent.copy()
                for s in slots_of(mask, use_map, use_rec):
                    want[s, :6] = sent[s, :6] + f[s, :6]
                    want[s, 6] = np.fmax(sent[s, 6], f[s, 6])
                if not np.array_equal(a.view(np.uint64), want.view(np.uint64)):
                    fails.append((mask, use_map, use_rec))
                if use_map and use_rec:   # the fresh launch itself against the exact oracle
                    emu, *_ = emulation_sums([Chunk(x=xd.cpu(), recorded=rd.cpu())], torch.from_numpy(w), formats_of(mask),
                                             torch.from_numpy(bias), images["map"])
                    bad = verdict(f, emu, grid_expect(x, w, bias, images, rd.float().cpu().numpy(), True, mask))
                    if bad:
                        fails.append((mask, "oracle", bad[:3]))
    assert not fails, fails


@gpu
@pytest.mark.parametrize("rec_dtype", [torch.bfloat16, torch.float32])
def test_strided_recorded(rec_dtype):
    """A recorded output with row stride > N gives the bits of a contiguous copy, and the exact oracle's sums."""
    torch.cuda.set_device(0)
    m, n, k = 130, 70, 48
    x, w, bias, amap, images, rec = grid_case(m, n, k, 13, 0xF, True, False, True, False)
    rec = rec + np.float32(0.5)                                    # still on the grid, and not R
    big = torch.zeros((m, n + 37), dtype=rec_dtype, device="cuda")
    big[:, 5: 5 + n] = torch.from_numpy(rec).to(rec_dtype)
    view = big[:, 5: 5 + n]
    assert view.stride(0) == n + 37
    xd, wd = torch.from_numpy(x).to(torch.bfloat16).cuda(), torch.from_numpy(w).to(torch.bfloat16).cuda()
    a = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
    b = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
    hb.output_error(xd, wd, 0xF, a, recorded=view)
    hb.output_error(xd, wd, 0xF, b, recorded=view.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    recv = view.float().cpu().numpy()
    emu, *_ = emulation_sums([Chunk(x=xd.cpu(), recorded=view.cpu())], wd.cpu(), FMTS, None)
    bad = verdict(a.cpu().numpy(), emu, grid_expect(x, w, None, images, recv, False, 0xF))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("special", ["nan_first", "nan_last", "inf"])
def test_atol_nan_and_inf_match_emulation(special, chunked):
    """A recorded output holding NaN (in the first or the last chunk) or ±Inf: the kernel's atol equals the emulation's (NaN with
    NaN, Inf with Inf); the other slots stay exact."""
    torch.cuda.set_device(0)
    m, n, k = 229, 70, 40
    x, w, bias, amap, images, rec = grid_case(m, n, k, 21, 0xF, False, False, True, True)
    rec = rec.astype(np.float32)
    if special == "inf":
        rec[3, 5], rec[200, 69] = np.inf, -np.inf
    else:
        rec[3 if special == "nan_first" else 228, 7] = np.nan
    got, want = run_both(x, w, bias, 0xF, None, images, rec, False, chunk_rows=128 if chunked else None)
    s = SLOTS.index("recorded")
    if special == "inf":
        assert got[s][6] == want[s][6] == np.inf
    else:
        assert np.isnan(got[s][6]) and np.isnan(want[s][6]), (got[s], want[s])
    bad = verdict(got, want, grid_expect(x, w, bias, images, rec, False, 0xF))
    assert not bad, bad
