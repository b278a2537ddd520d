"""The exact-arithmetic cases of the calibration kernels (csrc/mtq_budget.hip, csrc/mtq_gptq.hip; DESIGN.md, "The exact regime of
the calibration kernels"), built and proved exact on the host.  test_calibration_exact_gpu.py runs the same cases on the device and
asks for bit equality.

On these inputs every product and every partial sum of the float64 emulations is an integer multiple of one quantum below 2⁵³ quanta,
so the emulation's result does not depend on the summation order and is the one right answer:
  * Gram (mtq_gram_blocks, mtq_gram_full) — X small integers in bf16: bf16 products, f32 folds of at most 256 tokens (max|x|²·256 <
    2²⁴) and float64 sums are exact; the reference is XᵀX in int64;
  * tables (mtq_tile_error_tables, both layouts) — W small integers times one power of two per 16 × 16 block, H integer blocks: Δ is on
    a per-tile quantum and e_out, e_w are recomputed in int64 with Σ|term| < 2⁵³ quanta;
  * sweep (mtq_gptq_sweep) — W integers times a power of two per row, U = diag(2^s)·Z with Z unit upper triangular and integer: e_j·U_jj'
    = (w_j − q_j)·Z_jj' is an integer number of quanta; the reference is a restatement of gptq.py's sweep contract in int64 that
    takes only the element rule (gq.q_fixed) from the package, and counts the events the cases must contain (saturation, level ties,
    groups whose E comes from the CURRENT values)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.quantization_formats import quantize_weight_values

ALL = list(MIXED_TILE_FORMATS)
TILE = 32
GROUP = 16
FOLD = 256                                   # tokens per f32 → f64 fold (mtq.h: "folded into float64 at least every 256 tokens")
EXACT = 2 ** 53


# ----------------------------------------------------------------------------- Gram

X_MAX = 15
GRAM_K = [1, 31, 32, 33, 127, 128, 129, 160, 1000, 1024, 2048, 7168]
GRAM_M = [1, 63, 64, 65, 255, 256, 257, 511, 513]
GRAM_M_LARGE = 40000


def gram_ints(m: int, k: int, seed: int, device="cpu") -> torch.Tensor:
    """Integers 1 .. X_MAX with random signs, m × k int16 on `device`: no zero, so a lost or doubled token changes every entry's sum of
    squares."""
    g = torch.Generator(device=device).manual_seed(seed * 1000003 + m * 31 + k)
    mag = torch.randint(1, X_MAX + 1, (m, k), generator=g, device=device, dtype=torch.int16)
    return mag * (2 * torch.randint(0, 2, (m, k), generator=g, device=device, dtype=torch.int16) - 1)


def gram_tensor(xi: torch.Tensor) -> torch.Tensor:
    x = xi.to(torch.bfloat16)
    assert torch.equal(x.to(torch.int16), xi)                    # every value is a bf16
    return x


def gram_int(xi: np.ndarray) -> np.ndarray:
    return xi.T @ xi


def gram_block_int(xi: np.ndarray) -> np.ndarray:
    m, k = xi.shape
    nb = -(-k // TILE)
    xp = np.zeros((m, nb * TILE), dtype=np.int64)
    xp[:, :k] = xi
    xb = xp.reshape(m, nb, TILE)
    return np.einsum("mbi,mbj->bij", xb, xb)


def gram_spans(kind: str, m: int, k: int) -> int:
    """Token spans of one launch over (m, k), from the public scratch-size queries: mtq_gram_blocks keeps ceil(k/32) blocks per span,
    mtq_gram_full 16 blocks per pair of 128-column super blocks and span, and none at all for a single span."""
    if kind == "blocks":
        return hb.gram_blocks_scratch(m, k) // (-(-k // TILE) * TILE * TILE)
    sb = -(-k // 128)
    return max(1, hb.gram_full_scratch(m, k) // (sb * (sb + 1) // 2 * 16 * TILE * TILE))


def gram_span(kind: str, m: int, k: int) -> list:
    """The (span, spans) one launch over (m, k) may use: spans from the query, the span any whole number of folds with
    ceil(m / span) == spans.  Often one pair, a few where the spans are long."""
    spans = gram_spans(kind, m, k)
    return [(s, spans) for s in range(FOLD, (-(-m // FOLD) + 1) * FOLD, FOLD) if -(-m // s) == spans]


def gram_edge_ms(kind: str, k: int, m_hint: int = GRAM_M_LARGE) -> list:
    """(name, m, span, spans): token counts near m_hint whose last span holds 1 token, span − 1 tokens and a full span, for every span
    length the launch over m_hint tokens may use, each kept only if the query for that very m allows the same geometry.  Empty when a
    launch over m_hint tokens is a single span."""
    out = []
    for span, spans in gram_span(kind, m_hint, k):
        if spans < 2:
            continue
        for name, m in (("one", (spans - 1) * span + 1), ("span-1", spans * span - 1), ("full", spans * span)):
            if (span, spans) in gram_span(kind, m, k):
                out.append((name, m, span, spans))
    return out


def test_gram_cases_are_exact_and_the_emulations_equal_int64():
    assert X_MAX * X_MAX * FOLD < 2 ** 24                        # an f32 fold of 256 tokens holds every partial sum exactly
    assert X_MAX * X_MAX * (1 << 30) < EXACT                     # and float64 any number of tokens a test can hold
    for m, k in [(1, 1), (63, 31), (257, 33), (513, 129), (1000, 160), (300, 1000), (5000, 40)]:
        xt = gram_ints(m, k, 0)
        x = gram_tensor(xt)
        xi = xt.numpy().astype(np.int64)
        assert np.abs(xi).max() <= X_MAX and (xi != 0).all()
        cuts = [0, m // 3, m // 3, m]                            # an empty chunk among them
        chunks = [Chunk(x=x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        h, tokens = gq.gram_full_emulation(chunks, k)
        assert tokens == m and np.array_equal(h, gram_int(xi).astype(np.float64))
        hb_, tokens = bm.gram_blocks_emulation(chunks, k)
        assert tokens == m and np.array_equal(hb_, gram_block_int(xi).astype(np.float64))
        nb = -(-k // TILE)
        full = np.zeros((nb * TILE, nb * TILE), dtype=np.int64)
        full[:k, :k] = gram_int(xi)
        assert all(np.array_equal(gram_block_int(xi)[b], full[b * TILE:(b + 1) * TILE, b * TILE:(b + 1) * TILE]) for b in range(nb))


def test_gram_span_geometry_from_the_scratch_queries():
    """The shapes the device test relies on: each k has its span edges, mtq_gram_full at k = 1024 runs spans of several folds through
    scratch, and at k >= 5632 a single span without scratch (mtq.h)."""
    for k in GRAM_K:
        for kind in ("blocks", "full"):
            e = gram_edge_ms(kind, k)
            if kind == "full" and hb.gram_full_scratch(GRAM_M_LARGE, k) == 0:
                assert k >= 5632 and e == []
                continue
            assert {name for name, *_ in e} == {"one", "span-1", "full"}, (kind, k, e)
            for _name, m, span, spans in e:
                assert spans >= 2 and span % FOLD == 0 and (spans - 1) * span < m <= spans * span
    ((span, spans),) = gram_span("full", GRAM_M_LARGE, 1024)
    assert span > FOLD and spans > 1 and hb.gram_full_scratch(GRAM_M_LARGE, 1024) > 0
    assert gram_spans("full", 64, 18432) == 1 and hb.gram_full_scratch(64, 18432) == 0


# ----------------------------------------------------------------------------- tile error tables

TABLE_SHAPES = [(70, 100), (64, 96), (33, 7), (300, 200), (1, 1), (17, 33), (95, 31)]   # ragged last tiles in both directions
TABLE_LARGE = [(2417, 7168, "dense", "bf16"), (524330, 7, "gram", "f32")]   # more tile rows (columns) than the launch has workgroups in y
_BLOCK_SHIFT = (0, 1, 3, 2, 0, -3, 2, 1)
_TILE_SCALE = (0, -100, 70, -9, 5, 0, 12)


def tables_weight(n: int, k: int, seed: int, pad: int = 5) -> np.ndarray:
    """float32 n × (k + pad): integers in ±63 (bf16 values) times 2^s, s = a scale per 32 × 32 tile of the view [:, 2 : 2 + k] (0,
    tiny 2⁻¹⁰⁰, huge 2⁷⁰, ...) plus a shift per 16 × 16 block, so groups of either layout share a tile's quantum; one all-zero 16 × 16
    block.  A tile never mixes scales further apart than 2⁶: that, not a tolerance, keeps Σ δᵀHδ below 2⁵³ quanta."""
    rng = np.random.default_rng([n, k, seed])
    w = rng.integers(-63, 64, size=(n, k + pad)).astype(np.float64)
    r, c = np.arange(n)[:, None], (np.arange(k + pad)[None, :] - 2) % (k + pad)
    tile = (r // TILE) * 3 + c // TILE
    block = (r // GROUP) * 5 + c // GROUP
    s = np.take(_TILE_SCALE, tile % len(_TILE_SCALE)) + np.take(_BLOCK_SHIFT, block % len(_BLOCK_SHIFT))
    w = np.ldexp(w, s)
    w[(r // GROUP == 0) & (c // GROUP == (1 if k > GROUP else 0))] = 0.0
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    return w32


def tables_view(w32: np.ndarray, k: int, wdt: str, device="cpu") -> torch.Tensor:
    """The (n, k) view at column offset 2 of a (n, k + 5) tensor (ldw > k) on `device`, bf16 or float32 storage, both exact."""
    t = torch.from_numpy(w32).to(torch.bfloat16 if wdt == "bf16" else torch.float32)
    assert np.array_equal(t.float().numpy().view(np.uint32), w32.view(np.uint32))
    return t.to(device)[:, 2: 2 + k]


def tables_h(k: int, kind: str, seed: int) -> np.ndarray:
    """Integer Gram blocks [ceil(k/32), 32, 32] as float64: "gram" — XᵀX of integer X (|x| ≤ 7, 96 tokens); "dense" — an arbitrary
    symmetric integer H with off-diagonal entries as large as the diagonal, so a permuted δ row or column changes the answer."""
    rng = np.random.default_rng([k, seed, kind == "dense"])
    nb = -(-k // TILE)
    if kind == "gram":
        x = np.zeros((96, nb * TILE), dtype=np.int64)
        x[:, :k] = rng.integers(-7, 8, size=(96, k))
        xb = x.reshape(96, nb, TILE)
        return np.einsum("mbi,mbj->bij", xb, xb).astype(np.float64)
    a = rng.integers(-1000, 1001, size=(nb, TILE, TILE))
    return (a + a.transpose(0, 2, 1)).astype(np.float64)


def tables_quanta(w32: np.ndarray, f: str, layout: str):
    """Δ_f of budget_maps' contract in quanta → (di float64 [th, 32, tw, 32], integer valued; qe int [th, tw]): every tile on its own
    quantum 2^qe, the largest power of two that divides each δ of the tile."""
    n, k = w32.shape
    th, tw = bm.tiles_hw(n, k)
    q = quantize_weight_values(np.ascontiguousarray(w32.T), f).T if layout == "transpose" else quantize_weight_values(w32, f)
    d = np.zeros((th * TILE, tw * TILE))
    d[:n, :k] = q.astype(np.float64) - w32.astype(np.float64)
    dt = d.reshape(th, TILE, tw, TILE)                                        # [r, i, c, a]
    mm, ee = np.frexp(np.abs(dt))
    mi = np.ldexp(mm, 53).astype(np.int64)
    low = ee - 53 + np.frexp((mi & -mi).astype(np.float64))[1] - 1           # exponent of each δ's lowest set bit
    qe = np.where(dt != 0, low, 1 << 20).min(axis=(1, 3))
    qe = np.where(qe == 1 << 20, 0, qe)
    di = np.ldexp(dt, -qe[:, None, :, None])
    assert np.array_equal(di, np.rint(di)) and np.abs(di).max(initial=0) < 2.0 ** 40, f
    return di, qe


def tables_crude_bound(w32: np.ndarray, h: np.ndarray, layout: str) -> float:
    """32³ · max|δ|² · max|H| per tile, in quanta²: above Σ|δ_a||H_ab||δ_b| and Σδ² of the tile, so above every partial sum."""
    worst = 0.0
    hmax = np.abs(h).max(axis=(1, 2))
    for f in ALL:
        di, _qe = tables_quanta(w32, f, layout)
        worst = max(worst, float((np.abs(di).max(axis=(1, 3)) ** 2 * np.maximum(hmax, 1.0)[None, :]).max()) * TILE ** 3)
    return worst


def tables_int(w32: np.ndarray, h: np.ndarray, layout: str):
    """e_out and e_w of budget_maps' contract in int64 → (e_out, e_w, worst): float64 [T, 4] tables (integer · quantum², exact) and the
    largest Σ|term| of any tile in quanta², which bounds every partial sum of any summation order."""
    hi = h.astype(np.int64)
    assert np.array_equal(hi.astype(np.float64), h)
    th, tw = bm.tiles_hw(*w32.shape)
    e_out, e_w, worst = np.zeros((th * tw, 4)), np.zeros((th * tw, 4)), 0.0
    for code, f in enumerate(ALL):
        di, qe = tables_quanta(w32, f, layout)
        ad = np.abs(di)
        bound = np.einsum("ricb,ricb->rc", np.einsum("rica,cab->ricb", ad, np.abs(h)), ad)   # float64: a bound needs no last bit
        worst = max(worst, float(bound.max()) * (1 + 2.0 ** -40), float(np.einsum("rica,rica->rc", ad, ad).max()))
        assert worst < EXACT, (f, worst)
        di = di.astype(np.int64)
        so = np.einsum("ricb,ricb->rc", np.einsum("rica,cab->ricb", di, hi), di)
        sw = np.einsum("rica,rica->rc", di, di)
        out = np.ldexp(so.astype(np.float64), 2 * qe)
        ew = np.ldexp(sw.astype(np.float64), 2 * qe)
        e_out[:, code] = (out.T if layout == "transpose" else out).reshape(-1)
        e_w[:, code] = (ew.T if layout == "transpose" else ew).reshape(-1)
    return e_out, e_w, worst


@pytest.mark.parametrize("layout", ["rows", "transpose"])
@pytest.mark.parametrize("hkind", ["gram", "dense"])
@pytest.mark.parametrize("n,k", TABLE_SHAPES)
def test_table_cases_are_exact_and_the_emulation_equals_int64(n, k, hkind, layout):
    for wdt in ("bf16", "f32"):
        w = tables_view(tables_weight(n, k, 0), k, wdt)
        w32 = w.float().numpy()
        h = tables_h(k, hkind, 0)
        want_out, want_w, worst = tables_int(w32, h, layout)
        assert worst < EXACT
        got_out, got_w = bm.tile_error_tables_emulation(w, h, layout)
        assert np.array_equal(got_out.view(np.uint64), want_out.view(np.uint64))
        assert np.array_equal(got_w.view(np.uint64), want_w.view(np.uint64))
        assert np.isfinite(want_out).all() and np.isfinite(want_w).all()
        if n >= 64 and k >= 64:
            mags = want_w[:, 3][want_w[:, 3] > 0]
            assert mags.max() / mags.min() > 2.0 ** 300          # the tiny and the huge tile are both there


@pytest.mark.parametrize("n,k,hkind,wdt", TABLE_LARGE)
def test_large_table_cases_stay_below_2_53_quanta(n, k, hkind, wdt):
    """The shapes whose grid-stride loops iterate: each workgroup column walks more tiles than the launch has rows in y (16384 / tile
    columns, mtq_budget.hip).  Exactness by the crude per-tile bound alone; the device test forms their float64 reference on the device."""
    th, tw = bm.tiles_hw(n, k)
    assert th > 16384 // tw and th * tw * 4 < 1 << 22
    w32 = tables_view(tables_weight(n, k, 0), k, wdt).float().numpy()
    h = tables_h(k, hkind, 0)
    for layout in ("rows", "transpose"):
        assert tables_crude_bound(w32, h, layout) < EXACT


def test_dense_h_sees_a_swapped_pair_of_columns_inside_a_tile():
    """δ columns 3 and 4 of every tile exchanged (the same as H's rows and columns 3 and 4 exchanged): with the dense H every tile that
    has an error moves by far more than the 1e-12 of the rounding-bound tests."""
    n, k = 64, 96
    w32 = tables_view(tables_weight(n, k, 0), k, "f32").float().numpy()
    h = tables_h(k, "dense", 0)
    p = np.arange(TILE)
    p[[3, 4]] = p[[4, 3]]
    a, _aw, _ = tables_int(w32, h, "rows")
    b, _bw, _ = tables_int(w32, h[:, p][:, :, p], "rows")
    live = a[:, 3] != 0
    assert live.any() and np.all(np.abs(a[live, 3] - b[live, 3]) > 1e-6 * np.abs(a[live, 3]))


# ----------------------------------------------------------------------------- the sweep

SWEEP_Q = 24                                 # quantum 2⁻²⁴
SWEEP_SHAPES = [(1, 1), (31, 15), (33, 16), (1, 17), (31, 33), (33, 48), (70, 48), (70, 100), (33, 144), (70, 144), (31, 200), (70, 200),
                (33, 1000), (70, 1000)]
SWEEP_KINDS = ["bf16", "bfp8", "bfp4", "bfp2", "map"]
SWEEP_LONG = (4, 7168, "map")


def sweep_codes(n: int, k: int, kind: str) -> np.ndarray:
    if kind == "map":
        return np.random.default_rng([n, k]).integers(0, 4, size=(-(-n // TILE), -(-k // TILE))).astype(np.int8)
    return gq.constant_codes(n, k, kind)


def sweep_case(n: int, k: int, wdt: str = "bf16", seed: int = 0, pad: int = 3):
    """(w32 n × (k + pad), U k × k): W integers times a power of two per row — ±255 times 2⁻⁹ .. 2⁻⁶ for bf16 storage (every value a
    bf16; under bfp8 a group whose maximum has 8 bits puts every odd integer on a tie), ±1023 times 2⁻¹¹ .. 2⁻⁸ for float32 storage (so
    the bf16 code rounds too); U = diag(2^s)·Z, s in −2 .. 2, Z unit upper triangular with integer entries ±1, ±2 — about one in ten
    above the diagonal, at most about four per row of Z."""
    rng = np.random.default_rng([n, k, seed, wdt == "bf16"])
    top, lo = (255, -9) if wdt == "bf16" else (1023, -11)
    wi = rng.integers(-top, top + 1, size=(n, k + pad))
    salt = rng.random(wi.shape) < 0.125                          # one value in eight a power of two: half a BFP step of some group maximum,
    wi[salt] = (np.sign(wi[salt] + 0.5) * 2 ** rng.integers(3, 8 if top == 255 else 10, size=int(salt.sum()))).astype(np.int64)   # or the maximum
    w = np.ldexp(wi.astype(np.float64), rng.integers(lo, lo + 4, size=(n, 1)))
    dens = min(0.1, 4.0 / max(k, 1))
    u = np.zeros((k, k), dtype=np.float64)
    for j in range(k):
        cols = j + 1 + np.nonzero(rng.random(k - j - 1) < dens)[0]
        u[j, cols] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=cols.size)
        u[j, j] = 1.0
        u[j] = np.ldexp(u[j], int(rng.integers(-2, 3)))
    return w.astype(np.float32), u


FORCED_K = 96
FORCED_TARGETS = [5, 20, 40, 60]


def forced_case(code: int):
    """Built by hand for MIXED_TILE_FORMATS code 1..3 (M mantissa bits), 4 rows × 96 columns, values on the 2⁻⁹ grid: every group's
    maximum is 1 (E = 127, step = 2^(1−M)) and one column of each of the first four groups sits half a step above a level, so
    its error is ∓ step / 2 (an exact level tie).  A U entry of ±2^(M+3) times the diagonal from that column lifts a later column of the
    SAME group to about 8: its exponent field exceeds E, which was fixed at the group's start — saturation, in the first group of a
    block (columns 0 → 5, 33 → 40) and in the second (17 → 20, 50 → 60).  Column 3 is a tie too and Z[3, 85] = ±2^(M+5) lifts column 85,
    in the second group of the third block, before that group starts: its E comes from the CURRENT values (132, not 127).  Row 1 is
    negated, row 2 alternates signs and row 3 is halved (E = 126)."""
    m = gq._MANT[code]
    step = 2.0 ** (1 - m)
    w = np.full((4, FORCED_K), 0.25)
    w[:, 9::GROUP] = 1.0
    tie, q_tie = (3.5 * step, 4.0 * step) if m > 1 else (0.5, 0.0)   # half a step above an odd level (rounds up), M = 1: 0.5 → 0
    for a in (0, 17, 33, 50, 3):
        w[:, a] = tie
    w[1] = -w[1]
    w[2, 1::2] = -w[2, 1::2]
    w[3] *= 0.5
    z = np.eye(FORCED_K)
    for a, b in zip((0, 17, 33, 50), FORCED_TARGETS):
        z[a, b] = -8.0 / (tie - q_tie)                           # the target column gains 8 (in rows 0 .. 2)
    z[3, 85] = -32.0 / (tie - q_tie)
    z[1, 2] = z[20, 31] = z[60, 62] = z[70, 90] = 2.0
    u = np.ldexp(z, (np.arange(FORCED_K) % 5 - 2)[:, None])
    return w.astype(np.float32), u, gq.constant_codes(4, FORCED_K, ALL[code])


def sweep_view(w32: np.ndarray, k: int, wdt: str, device="cpu") -> torch.Tensor:
    """The (n, k) view at column offset 1 of the (n, k + pad) tensor on `device` (ldw > k; the tensor itself when pad = 0), bf16 or
    float32 storage, both exact."""
    t = torch.from_numpy(w32).to(torch.bfloat16 if wdt == "bf16" else torch.float32)
    assert np.array_equal(t.float().numpy().view(np.uint32), w32.view(np.uint32))
    t = t.to(device)
    return t[:, 1: 1 + k] if w32.shape[1] > k else t


def _exp_field32(v: np.ndarray) -> np.ndarray:
    """Exponent field of float32(v · 2⁻Q) for int64 quanta v, |v| < 2⁵³ (the int → float64 → float32 casts are NumPy's)."""
    f = np.ldexp(v.astype(np.float64), -SWEEP_Q).astype(np.float32)
    return ((f.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)


def sweep_int(w32: np.ndarray, u: np.ndarray, codes: np.ndarray):
    """gptq.py's sweep contract restated in int64 quanta of 2⁻²⁴, one column at a time (no blocking): → (Ŵ float32, loss float64,
    events).  Only q_E comes from the package.  events: per MIXED_TILE_FORMATS code the number of saturated elements, exact level ties
    and groups whose E differs from that of the original weights; "worst" the largest Σ|term| of any value's history in quanta (it
    bounds every partial sum of every summation order) and "loss_worst" the largest loss in quanta of the loss (the largest
    power of two that divides every e²)."""
    n, k = w32.shape
    scale = np.ldexp(w32.astype(np.float64), SWEEP_Q)
    assert np.array_equal(scale, np.rint(scale)) and np.abs(scale).max(initial=0) < 2.0 ** 52
    w = scale.astype(np.int64)
    w0 = w.copy()
    mag = np.abs(w)                                              # Σ|term| of each value's history
    assert not np.tril(u, -1).any()                              # nothing below the diagonal
    mant, ex = np.frexp(np.diag(u))
    assert np.all(mant == 0.5)                                   # U_jj = 2^s_j
    s = ex.astype(np.int64) - 1
    crow = np.repeat(np.asarray(codes, dtype=np.int64), TILE, axis=0)[:n]
    q = np.zeros((n, k), dtype=np.float32)
    d = np.zeros((n, k), dtype=np.int64)
    ev = {c: {"saturated": 0, "ties": 0, "current_e": 0} for c in (1, 2, 3)}
    E = np.zeros(n, dtype=np.int64)
    mant_bits = np.array([0, 7, 3, 1])
    for j in range(k):
        f = crow[:, j // TILE]
        if j % GROUP == 0:
            E = _exp_field32(w[:, j: min(k, j + GROUP)]).max(axis=1)
            E0 = _exp_field32(w0[:, j: min(k, j + GROUP)]).max(axis=1)
            for c in ev:
                ev[c]["current_e"] += int(np.count_nonzero((f == c) & (E != E0)))
        v = w[:, j]
        qj = gq.q_fixed(np.ldexp(v.astype(np.float64), -SWEEP_Q), f, E)
        qi = np.ldexp(qj.astype(np.float64), SWEEP_Q)
        assert np.array_equal(qi, np.rint(qi))                   # q is a whole number of quanta
        qi = qi.astype(np.int64)
        ef = _exp_field32(v)
        step_e = E - 126 - mant_bits[f] + SWEEP_Q                # log2 of the BFP step in quanta
        for c in ev:
            sel = f == c
            ev[c]["saturated"] += int(np.count_nonzero(sel & (ef > E)))
            ok = sel & (ef <= E) & (E > 0) & (step_e >= 1) & (step_e < 62)
            half = np.left_shift(1, np.clip(step_e - 1, 0, 61))
            ev[c]["ties"] += int(np.count_nonzero(ok & ((np.abs(v) & (2 * half - 1)) == half)))
        d[:, j] = v - qi
        q[:, j] = qj
        nz = np.nonzero(u[j, j + 1:])[0] + j + 1
        if nz.size:
            zf = np.ldexp(u[j, nz], -int(s[j]))                  # Z_jj' = U_jj' / U_jj, an integer
            assert np.array_equal(zf, np.rint(zf)) and np.abs(zf).max() < 2 ** 20
            zj = zf.astype(np.int64)
            w[:, nz] -= d[:, j: j + 1] * zj[None, :]
            mag[:, nz] += np.abs(d[:, j: j + 1]) * np.abs(zj)[None, :]
    worst = int(mag.max(initial=0))
    assert worst < 2 ** 52, worst
    # loss_r = Σ_j (d_rj · 2^−s_j)² · 2⁻⁴⁸ in Python integers on the quantum 2^(−48 − 2·max s)
    smax = int(s.max())
    lq = [sum(int(x) ** 2 << int(2 * (smax - sj)) for x, sj in zip(row, s)) for row in d]
    low = functools.reduce(lambda a, b: a | b, [int(x) ** 2 << int(2 * (smax - sj)) for row in d for x, sj in zip(row, s)], 0)
    tz = (low & -low).bit_length() - 1 if low else 0             # every term is a multiple of 2^tz: the loss's own quantum
    ev["worst"], ev["loss_worst"] = worst, max(lq, default=0) >> tz
    assert ev["loss_worst"] < EXACT, ev["loss_worst"]
    loss = np.array([np.ldexp(float(x), -2 * SWEEP_Q - 2 * smax) for x in lq], dtype=np.float64)
    return q, loss, ev


def _assert_sweep_exact(w, u, codes, blocks):
    w32 = w.float().numpy()
    q, loss, ev = sweep_int(w32, u, codes)
    margins = None
    for block in blocks:
        got, got_loss, margins = gq.sweep_emulation(w, u, codes, block=block)
        assert np.array_equal(got.view(np.uint32), q.view(np.uint32)), block
        assert np.array_equal(got_loss.view(np.uint64), loss.view(np.uint64)), block
    return ev, margins


def sweep_family() -> list:
    """(n, k, storage, kind) of the random cases: every shape with every kind, bf16 and float32 storage alternating."""
    return [(n, k, "bf16" if (i + j) % 2 else "f32", kind) for i, (n, k) in enumerate(SWEEP_SHAPES) for j, kind in enumerate(SWEEP_KINDS)]


@functools.lru_cache(maxsize=None)
def _family_events():
    """Events and emulation margins over the whole family of random cases (every shape and kind; bf16 and f32 storage alternate)."""
    total = {c: {"saturated": 0, "ties": 0, "current_e": 0} for c in (1, 2, 3)}
    tied = rows = 0
    for n, k, wdt, kind in sweep_family():
        w32, u = sweep_case(n, k, wdt)
        ev, margin = _assert_sweep_exact(sweep_view(w32, k, wdt), u, sweep_codes(n, k, kind), (32, 128) if k > 32 else (16, max(k, 1)))
        for c in total:
            for key in total[c]:
                total[c][key] += ev[c][key]
        tied += int(np.count_nonzero(margin <= 2.0 ** -20))
        rows += n
    return total, tied, rows


def test_sweep_family_is_exact_at_several_block_sizes_and_lives_on_the_ties():
    total, tied, rows = _family_events()
    # the rows test_sweep_matches_emulation_on_clear_rows leaves out are the ones compared here
    assert tied >= 0.5 * rows, (tied, rows)
    for c in (1, 2, 3):
        assert total[c]["ties"] > 0 and total[c]["current_e"] > 0, (ALL[c], total[c])


@pytest.mark.parametrize("code", [1, 2, 3])
def test_forced_case_saturates_in_both_groups_of_a_block(code):
    w32, u, codes = forced_case(code)
    for wdt in ("bf16", "f32"):
        ev, margin = _assert_sweep_exact(sweep_view(w32, FORCED_K, wdt), u, codes, (16, 32, FORCED_K))
        assert ev[code]["saturated"] >= 16 and ev[code]["ties"] >= 20 and ev[code]["current_e"] >= 4, ev
        assert (margin <= 2.0 ** -20).all()
    q, _loss, _ev = sweep_int(w32, u, codes)
    m = gq._MANT[code]
    top = (2 ** m - 1) * 2.0 ** (1 - m)                          # E = 127: ±(2^M − 1)·step, in both groups of both blocks
    assert np.array_equal(np.abs(q[:3, FORCED_TARGETS]), np.full((3, 4), top, np.float32))
    assert np.array_equal(np.abs(q[3, FORCED_TARGETS]), np.full(4, top / 2, np.float32))
    assert np.array_equal(np.signbit(q[:, FORCED_TARGETS]), np.array([[False] * 4, [True] * 4, [False, True, True, False], [False] * 4]))


def test_family_and_forced_cases_hold_every_event_for_every_format():
    total, _tied, _rows = _family_events()
    for code in (1, 2, 3):
        _q, _l, ev = sweep_int(*forced_case(code))
        for key in ("saturated", "ties", "current_e"):
            assert total[code][key] + ev[code][key] > 0, (ALL[code], key)
        assert ev[code]["saturated"] > 0


def test_long_case_is_exact():
    n, k, kind = SWEEP_LONG
    w32, u = sweep_case(n, k, "bf16")
    ev, margin = _assert_sweep_exact(sweep_view(w32, k, "bf16"), u, sweep_codes(n, k, kind), (32, k))
    assert (margin <= 2.0 ** -20).mean() >= 0.5 and ev["worst"] < 2 ** 40
