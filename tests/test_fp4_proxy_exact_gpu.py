"""The sums of mtq_fp4_proxy_sums (csrc/mtq_fp4_proxy.hip) on inputs where they are exact, on every launch path.

x = k / 64 with integers |k| ≤ 255: bf16-exact, reaching both scale branches of nvfp4; for both proxies every term the kernel forms
in float32 (x, x², y, y², xy, |x − y|) equals its float64 value and is a multiple of 2⁻²⁰ below 32 in magnitude, so while a matrix
has fewer than 2²⁸ elements every float64 partial sum is exact, in any order.  The kernel's seven sums must then equal
Σₖ countₖ · termₖ over the 511 values bit for bit, with no ε, whatever G (partial-sum blocks per matrix), load path or batch
layout the launch takes.  The preconditions are asserted on the host (test_grid_preconditions runs without a GPU) and again for
every case (n < 2²⁸).  Padding the kernel must not read holds NaN, so a read past a row or a matrix shows."""
from __future__ import annotations

import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import quantization_formats as qf
from tests.inputs import gen

PROXIES = hb.PROXY_FORMATS
KMAX = 255
STEP = 1.0 / 64                      # the grid of x
UNIT = 2.0 ** -20                    # the grid of every term
N_MAX = 1 << 28                      # elements per matrix below which every float64 partial sum of terms is exact
ELEMS_PER_BLOCK = 32768              # csrc/mtq_fp4_proxy.hip kProxyElemsPerBlock
MASKS = [1, 2, 3]
STORAGE = {"bf16": torch.bfloat16, "f32": torch.float32}
gpu = pytest.mark.gpu


# ----------------------------------------------------------------------------- the exact host reference


def blocks_per_matrix(rows: int, cols: int) -> int:
    """G of csrc/mtq_fp4_proxy.hip blocks_per_matrix."""
    return max(1, min(rows, -(-rows * cols // ELEMS_PER_BLOCK)))


def float32_terms(x: np.ndarray, fmt: str) -> np.ndarray:
    """[len(x), 6] float64: x, x², y, y², xy, |x − y| formed in float32 from the emulation's y, as the kernel forms them."""
    x = np.asarray(x, np.float32)
    y = qf.quantize_weight_values(x, fmt)
    return np.stack([x, x * x, y, y * y, x * y, np.abs(x - y)], axis=1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def term_table(fmt: str) -> np.ndarray:
    """float32_terms of the 511 grid values k / 64, k = -255..255 (row k + 255), after checking what makes sums of them exact: each
    float32 term equals its float64 value and is a multiple of 2⁻²⁰ with |term| < 32."""
    k = np.arange(-KMAX, KMAX + 1)
    x = (k * STEP).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), k * STEP)
    t = float32_terms(x, fmt)
    x64, y64 = x.astype(np.float64), qf.quantize_weight_values(x, fmt).astype(np.float64)
    exact = np.stack([x64, x64 * x64, y64, y64 * y64, x64 * y64, np.abs(x64 - y64)], axis=1)
    assert np.array_equal(t, exact), f"{fmt}: a float32 term of the grid is not its float64 value"
    assert np.array_equal(t / UNIT, np.round(t / UNIT)) and np.abs(t).max() < 32, f"{fmt}: a term leaves the 2^-20 grid or the bound"
    return t


def exact_sums(counts: np.ndarray, mask: int) -> np.ndarray:
    """[2, 7] float64: Σ countₖ · termₖ per proxy in the mask (the unrequested slot stays 0), with max|x − y| over the values that
    occur.  Each product countₖ · termₖ and every partial sum is exact (n < 2²⁸), so this is the exact sum."""
    counts = np.asarray(counts, np.int64)
    assert counts.shape == (2 * KMAX + 1,) and counts.min() >= 0 and counts.sum() < N_MAX
    out = np.zeros((2, 7))
    for f, fmt in enumerate(PROXIES):
        if mask >> f & 1:
            t = term_table(fmt)
            out[f, :2] = counts @ t[:, :2]
            out[f, 2:6] = counts @ t[:, 2:6]
            out[f, 6] = t[counts > 0, 5].max(initial=0.0)
    return out


def grid_counts(k: np.ndarray) -> np.ndarray:
    return np.bincount(np.asarray(k, np.int64).ravel() + KMAX, minlength=2 * KMAX + 1)


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ----------------------------------------------------------------------------- device tensors and launch paths


class Case:
    """count matrices of rows × cols grid values k / 64, each a view into a (count, rows + row_pad, ld) NaN-filled buffer at column
    `offset`: stride_elems = (rows + row_pad) · ld, rows at a pitch of ld."""

    def __init__(self, count, rows, cols, ld=None, offset=0, row_pad=0, seed=0):
        ld = cols + offset if ld is None else ld
        assert ld >= cols + offset
        self.count, self.rows, self.cols, self.offset = count, rows, cols, offset
        rng = np.random.default_rng(seed)
        self.k = rng.integers(-KMAX, KMAX + 1, size=(count, rows, cols), dtype=np.int16)
        self.wide = np.full((count, rows + row_pad, ld), np.nan, np.float32)
        self.fill()

    def fill(self):
        self.wide[:, :self.rows, self.offset:self.offset + self.cols] = self.k.astype(np.float32) * np.float32(STEP)

    def device(self, storage: str, squeeze: bool = True):
        t = torch.from_numpy(self.wide).cuda().to(STORAGE[storage])   # exact: grid values are bf16 values, NaN stays NaN
        v = t[:, :self.rows, self.offset:self.offset + self.cols]
        return v[0] if squeeze and self.count == 1 else v

    def want(self, mask: int) -> np.ndarray:
        """[count, 2, 7]"""
        return np.stack([exact_sums(grid_counts(self.k[m]), mask) for m in range(self.count)])


def load_path(v) -> str:
    """Which load path of fp4_proxy_partials a launch on v takes, by the `vec` condition of mtq_fp4_proxy_sums: 'vector' (16-byte
    pieces only), 'tail' (16-byte pieces and a per-element row tail) or 'scalar' (per element)."""
    _code, count, stride, _rows, cols, ld = hb._matrix(v)
    esz = v.element_size()
    vec = v.data_ptr() % 16 == 0 and (ld * esz) % 16 == 0 and (count == 1 or (stride * esz) % 16 == 0)
    return "scalar" if not vec else ("tail" if cols % (16 // esz) else "vector")


def run(v, mask: int) -> np.ndarray:
    out = hb.fp4_proxy_sums(v, [f for i, f in enumerate(PROXIES) if mask >> i & 1]).cpu().numpy()
    return out.reshape(-1, 2, 7)


def check_exact(case: Case, storage: str, masks=MASKS) -> None:
    v = case.device(storage)
    for mask in masks:
        got, want = run(v, mask), case.want(mask)
        assert same_bits(got, want), (storage, mask, np.argwhere(got.view(np.int64) != want.view(np.int64))[:4], got, want)


# ----------------------------------------------------------------------------- host: the preconditions


def test_grid_preconditions():
    """The term grid (term_table's asserts), both nvfp4 scale branches among the grid values, and the bound on n that the cases use."""
    for fmt in PROXIES:
        term_table(fmt)
    x = (np.arange(1, KMAX + 1) * STEP).astype(np.float32)
    e = qf._log2_floor_ceil((x / np.float32(6.0)).astype(np.float32))[0]
    assert (e < -6).any() and ((e >= -6) & (e <= 7)).any()
    assert 32.0 * N_MAX / UNIT <= 2.0 ** 53        # |partial sum| < 32 · n stays within float64's 2^53 units of 2^-20
    assert 14339 * 4096 < N_MAX and blocks_per_matrix(14339, 4096) == 1793


# ----------------------------------------------------------------------------- GPU: G, load paths, batches


G_SHAPES = {   # rows, cols, ld, G: rows not a multiple of G, rows 16-byte aligned (ld), cols ragged where it says so
    "G1": (37, 500, 504, 1),
    "G1-vector-row": (1, 200003, 200008, 1),
    "G63": (1000, 2064, 2064, 63),
    "G64": (1000, 2097, 2104, 64),
    "G65": (1000, 2129, 2136, 65),
    "G129": (1000, 4227, 4232, 129),
    "G1793": (14339, 4096, 4096, 1793),
}


@gpu
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("name", list(G_SHAPES))
def test_exact_sums_across_G(storage, name):
    """fp4_proxy_finish takes G partials per matrix: lane ℓ adds blocks ℓ, ℓ + 64, ...; G > 64 runs its loop more than once."""
    rows, cols, ld, G = G_SHAPES[name]
    assert blocks_per_matrix(rows, cols) == G and (G == 1 or rows % G)
    check_exact(Case(1, rows, cols, ld=ld, seed=G), storage)


PATHS = {   # rows, cols, ld, offset, path
    "vector": (1000, 4224, 4224, 0, "vector"),
    "tail": (1000, 4227, 4232, 0, "tail"),
    "scalar-unaligned": (1000, 4227, 4232, 1, "scalar"),
    "scalar-ld": (3000, 77, 77, 0, "scalar"),
}


@gpu
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("path", list(PATHS))
def test_exact_sums_on_every_load_path(storage, path):
    rows, cols, ld, offset, want_path = PATHS[path]
    case = Case(1, rows, cols, ld=ld, offset=offset, seed=7)
    assert load_path(case.device(storage)) == want_path
    check_exact(case, storage)


# a batch: G = 65 with rows a multiple of G, so the last row of every matrix is the last block's; cols ragged (a row tail); three
# NaN rows between matrices, so stride_elems is larger than one matrix
BATCH = dict(count=5, rows=650, cols=3275, ld=3280, row_pad=3)


def batch_case(seed=11, count=BATCH["count"]) -> Case:
    c = Case(**{**BATCH, "count": count}, seed=seed)
    G = blocks_per_matrix(c.rows, c.cols)
    assert G == 65 and c.rows % G == 0 and (c.rows - 1) % G == G - 1
    return c


@gpu
@pytest.mark.parametrize("storage", list(STORAGE))
def test_exact_sums_of_a_batch(storage):
    case = batch_case()
    v = case.device(storage)
    assert load_path(v) == "tail" and hb._matrix(v)[2] > (case.rows - 1) * v.stride(1) + case.cols
    check_exact(case, storage)


@gpu
@pytest.mark.parametrize("storage", list(STORAGE))
def test_one_grid_step_shows(storage):
    """Moving one element by one grid step, at the very last element of the batch and inside a row tail of a middle matrix, moves Σx
    of that matrix by exactly 1/64 and leaves the others alone: the comparison above can fail."""
    case = batch_case()
    base = run(case.device(storage), 3)
    V = 16 // torch.empty((), dtype=STORAGE[storage]).element_size()
    tail0 = case.cols - case.cols % V
    for m, r, c in ((case.count - 1, case.rows - 1, case.cols - 1), (2, 301, tail0 + 1)):
        assert c >= tail0
        k0 = int(case.k[m, r, c])
        step = 1 if k0 < KMAX else -1
        case.k[m, r, c] = k0 + step
        case.fill()
        got = run(case.device(storage), 3)
        assert same_bits(got, case.want(3)), (m, r, c)
        assert (got[m, :, 0] - base[m, :, 0] == step * STEP).all()
        others = [i for i in range(case.count) if i != m]
        assert same_bits(got[others], base[others])
        case.k[m, r, c] = k0
        case.fill()


# ----------------------------------------------------------------------------- GPU: NaN and ±Inf, zeros and subnormals


@functools.lru_cache(maxsize=None)
def special_columns(special: float, where: str) -> tuple:
    """columns_from_sums of the emulation's float64 sums (host_sums of test_fp4_proxy_gpu) of the matrix that holds the special."""
    from tests.test_fp4_proxy_gpu import host_sums

    case, (m, r, c) = special_case(special, where)
    x = case.k[m].astype(np.float32) * np.float32(STEP)
    x[r, c] = special
    return tuple(tuple(hb.columns_from_sums(host_sums(x, f), x.size)[k] for k in ("pcc", "mae", "atol")) for f in PROXIES)


def special_case(special: float, where: str):
    case = batch_case(seed=5, count=3)
    G = blocks_per_matrix(case.rows, case.cols)
    # tail: a row tail of a row of block 3; last: the last row (block G - 1, the finish loop's second pass), a 16-byte piece
    at = (1, 3, case.cols - 2) if where == "tail" else (1, case.rows - 1, 5)
    assert where != "tail" or at[2] >= case.cols - case.cols % 4
    assert where != "last" or at[1] % G == G - 1 and G > 64
    return case, at


@gpu
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("where", ["tail", "last"])
@pytest.mark.parametrize("special", [float("nan"), float("inf"), float("-inf")], ids=["nan", "+inf", "-inf"])
def test_specials_stay_in_their_matrix(storage, where, special):
    """y of NaN and ±Inf is NaN in both proxies: Σy, Σy², Σxy, Σ|x − y| and max|x − y| of that matrix are NaN (nan_max in the lane,
    across the waves and in the finish), Σx and Σx² follow IEEE, the other matrices of the batch keep their bits, and the columns
    are NaN as the emulation's are."""
    case, (m, r, c) = special_case(special, where)
    clean = case.device(storage)
    case.wide[m, r, case.offset + c] = special
    dirty = case.device(storage)
    want_x = np.nan if np.isnan(special) else special
    want_x2 = np.nan if np.isnan(special) else np.inf
    others = [i for i in range(case.count) if i != m]
    for mask in MASKS:
        base, got = run(clean, mask), run(dirty, mask)
        assert same_bits(got[others], base[others]), mask
        for f in range(2):
            if not mask >> f & 1:
                assert not got[:, f].any()
                continue
            s = got[m, f]
            assert np.isnan(s[2:]).all(), (mask, f, s)
            assert np.isnan(s[0]) if np.isnan(want_x) else s[0] == want_x, s
            assert np.isnan(s[1]) if np.isnan(want_x2) else s[1] == want_x2, s
            cols = hb.columns_from_sums(s, case.rows * case.cols)
            host = special_columns(special, where)[f]
            for j, key in enumerate(("pcc", "mae", "atol")):
                assert np.isnan(cols[key]) and np.isnan(host[j]), (key, cols[key], host[j])


@gpu
def test_zeros_and_subnormals_leave_the_exact_sums():
    """±0 and float32 subnormals among the grid values (float32 storage, G = 65, a row tail): their squares and products are 0 in
    float32, and x, y, |x − y| of them are below 2⁻¹²⁶, far under half an ulp of any nonzero float64 multiple of 2⁻²⁰.  So each
    partial sum is the exact grid sum, or tiny where that is zero, and every slot whose grid sum is nonzero must equal it bit for
    bit; max|x − y| is the grid maximum."""
    case = batch_case(seed=23)
    rng = np.random.default_rng(29)
    special = rng.random((case.count, case.rows, case.cols)) < 0.2
    bits = rng.integers(0, 1 << 23, size=special.sum(), dtype=np.uint32) | (rng.integers(0, 2, size=special.sum(), dtype=np.uint32) << 31)
    tiny = bits.view(np.float32)                                      # subnormals, ±0 (one in 2^23) and some explicit ±0 below
    tiny[::97], tiny[1::97] = np.float32(0.0), np.float32(-0.0)
    case.wide[:, :case.rows, case.offset:case.offset + case.cols][special] = tiny
    t_terms = {fmt: float32_terms(tiny, fmt) for fmt in PROXIES}
    for fmt, t in t_terms.items():
        assert not t[:, [1, 3, 4]].any(), fmt                         # squares and products underflow to 0 in float32
        assert np.abs(t).max() <= 2.0 ** -126 and t.shape[0] * 2.0 ** -126 < 2.0 ** -74
    got = run(case.device("f32"), 3)
    for m in range(case.count):
        want = exact_sums(grid_counts(case.k[m][~special[m]]), 3)
        assert (want[:, :6] != 0).all(), "a grid sum is zero: pick another seed"
        assert same_bits(got[m], want), (m, got[m], want)


# ----------------------------------------------------------------------------- GPU: a large tensor, and batches past one launch


def emulation_sums_threaded(x: np.ndarray, fmt: str) -> np.ndarray:
    """host_sums of test_fp4_proxy_gpu by row chunks on a few threads (NumPy releases the GIL), float64 throughout."""
    parts = np.array_split(np.arange(x.shape[0]), 64)

    def part(ix):
        xs = x[ix[0]:ix[-1] + 1]
        t = float32_terms(xs.ravel(), fmt)
        return np.concatenate([t.sum(axis=0), [t[:, 5].max()]])

    workers = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))
    with ThreadPoolExecutor(workers) as pool:
        p = np.stack(list(pool.map(part, parts)))
    return np.concatenate([p[:, :6].sum(axis=0), [p[:, 6].max()]])


@gpu
def test_heavy_tailed_f32_at_G1792():
    """Not exact: a heavy-tailed float32 14336 × 4096 tensor (G = 1792) against the emulation's float64 sums, with the tolerances of
    test_sums_match_the_emulation_columns."""
    rows, cols = 14336, 4096
    assert blocks_per_matrix(rows, cols) == 1792
    x = gen("heavy_f32", 1792, (rows, cols))
    got = hb.fp4_proxy_sums(torch.from_numpy(x).cuda(), PROXIES).cpu().numpy()
    for i, fmt in enumerate(PROXIES):
        want = emulation_sums_threaded(x, fmt)
        np.testing.assert_allclose(got[i][:6], want[:6], rtol=1e-12, atol=0)
        assert got[i][6] == want[6]
        c, w = hb.columns_from_sums(got[i], x.size), hb.columns_from_sums(want, x.size)
        assert abs(c["pcc"] - w["pcc"]) <= 1e-12 and abs(c["mae"] - w["mae"]) <= 1e-12 * w["mae"] and c["atol"] == w["atol"]


@gpu
def test_more_matrices_than_one_launch():
    """(70000, 16, 16) float32: more than the 65535 matrices one launch of mtq_fp4_proxy_sums takes.  On grid values every matrix
    must equal its exact sums, which a single-matrix launch gives (G = 1, covered above); the first and last matrix of each launch,
    and a sample, equal their own single-matrix launches bit for bit, on grid values and on heavy-tailed ones."""
    count, rows, cols = 70000, 16, 16
    assert count > hb.PROXY_MAX_COUNT and blocks_per_matrix(rows, cols) == 1
    rng = np.random.default_rng(70000)
    k = rng.integers(-KMAX, KMAX + 1, size=(count, rows, cols), dtype=np.int16)
    x = torch.from_numpy(k.astype(np.float32) * np.float32(STEP)).cuda()
    got = hb.fp4_proxy_sums(x, PROXIES).cpu().numpy()
    idx = k.astype(np.int32) + KMAX
    for f, fmt in enumerate(PROXIES):
        table = term_table(fmt)
        want = np.empty((count, 7))
        for j in range(6):                                             # exact in any order: n = 256 terms per matrix
            want[:, j] = table[:, j][idx].sum(axis=(1, 2))
        want[:, 6] = table[:, 5][idx].max(axis=(1, 2))
        assert same_bits(got[:, f], want), np.argwhere((got[:, f] != want).any(axis=1))[:8].ravel()
    M = hb.PROXY_MAX_COUNT
    pick = sorted({0, M - 1, M, count - 1, *rng.choice(count, 64, replace=False).tolist()})
    heavy = torch.from_numpy(gen("heavy_f32", 16, (count, rows, cols))).cuda()
    got_heavy = hb.fp4_proxy_sums(heavy, PROXIES).cpu()
    for xb, gb in ((x, torch.from_numpy(got)), (heavy, got_heavy)):
        for i in pick:
            one = hb.fp4_proxy_sums(xb[i], PROXIES).cpu()
            assert torch.equal(gb[i].view(torch.int64), one.view(torch.int64)), i
