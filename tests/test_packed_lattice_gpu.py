"""GPU: the packed kernels of csrc/mtq_packed.hip over a lattice of shapes around every block, tile and step boundary, held to exact
arithmetic.  The other packed modules sit on hand-picked shapes with k >= 64 and a ragged n; here

  k in 1, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 256, 384
        1, 2, 3, 4 and 6 K steps of 64 (the wide kernel's one-step path, where the main loop is skipped and the odd tail multiplies
        from image 0; an even count above 2, where the last step runs with nothing left to stage), one tile column (k <= 32), a ragged
        group, a ragged piece of 8, k % 8 == 0 (16-byte loads of a contiguous X) beside k % 8 != 0;
  n in 1, 31, 32, 33, 64, 65, 127, 128, 129, 256          one output, whole and ragged tile rows, whole N blocks of 64 and of 128;
  m in 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256      the first m rows of one 256-row X: whole M blocks, one row past them.

References: Ŵ from the oracle (expected_bits) and Y from the float64 product on the integer grid of tests/packed_cases.py, whose
preconditions are asserted for every (n, k, map) over all 256 rows of X: every partial sum is a multiple of 2⁻⁸ below 2¹⁶ (at k <= 384
at most 4·384·256 + 255 < 2¹⁹ grid units), so f32 accumulation is exact in any order and every comparison is an equality.  Maps: random
over the four codes, and uniform bfp4.

  * block and wide at every m, float32 and bf16 Y, with and without bias, X contiguous and (at k % 8 == 0 and k = 1, 7, 33) at a pitch
    with an unaligned first element: each EQUALS the float64 product, the bf16 Y has the bits of the once-rounded exact float32 value,
    and the wide kernel's Y has the block kernel's bits;
  * skinny at m <= 32 and splits 0, 1, 2 and tiles_w + 1: the same, and split 0 is bit for bit the explicit split that the workspace
    size implies;
  * grouped: three experts of one pack_batch arena, group_rows (0, 0, 1, 33) and (31, 32, 65, 65) over 65 rows (groups of 0, 1, 32 and
    of 1, 33, 0 rows: an empty group first and last, one chunk, a chunk loop of 32 + 1, rows of no group), splits 0 and 2;
  * unpack of every packed W(n, k), float32 bit for bit and bf16 by upper halves, into sentinel-framed pitched buffers (one on the
    16-byte store path, one not) whose frame stays;
  * specials (Inf, NaN, denormals, exponent bytes 0 and 255): the wide kernel is the block kernel bit for bit, NaN where it has NaN;
  * one-hot: X = 2ˢ·I at k = m = 64, n = 128 (one step, whole blocks) and k = m = 256, n = 129 (four steps): every (n, k) position is
    the oracle's Ŵ, and one flipped bfp8 code byte (in the four-step case of the last step's tile column) shows at its position alone.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import GRID, _grid_case, _grid_preconditions, expected_bits, random_map, specials, uniform_map

pytestmark = pytest.mark.gpu

KS = (1, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 256, 384)
NS = (1, 31, 32, 33, 64, 65, 127, 128, 129, 256)
MS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256)
ROWS = max(MS)
PITCHED_KS = tuple(k for k in KS if k % 8 == 0 or k in (1, 7, 33))
GROUPED_KS = (1, 31, 32, 33, 64, 65, 128, 192)
GROUPED_NS = (1, 32, 33, 65, 129)
GROUPED_ROWS = ((0, 0, 1, 33), (31, 32, 65, 65))
GROUPED_T = 65
WHICH = ("random", "bfp4")
DTYPES = (torch.float32, torch.bfloat16)
SENTINEL = -7.0


def _what(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """Ŵ as float64, from the oracle."""
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _must_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if not torch.equal(got, want):
        raise AssertionError((what, "first mismatches at", (got != want).nonzero()[:4].tolist()))


def _map(n, k, which, seed=0):
    return random_map((n, k), n + k + seed) if which == "random" else uniform_map((n, k), 2)


@functools.lru_cache(maxsize=None)
def _x(k):
    """One 256-row X of the integer grid per k: (host float32, device bf16 contiguous, device bf16 at a pitch with an unaligned first
    element — tests/test_packed_wide_gpu.py's view) — made once, never written to."""
    x = _grid_case(ROWS, 1, k, 7000 + k)[0]
    assert np.array_equal(to_bf16_valued(x), x)
    xd = torch.from_numpy(x).to(torch.bfloat16).cuda()               # before x is made read-only
    buf = torch.zeros((ROWS, k + 9), dtype=torch.bfloat16, device="cuda")
    buf[:, 1:1 + k] = xd
    view = buf[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == k + 9                       # the scalar load path
    x.setflags(write=False)
    return x, xd, view


def _layouts(k):
    _x_host, xd, view = _x(k)
    return (("contiguous", xd), ("pitched", view)) if k in PITCHED_KS else (("contiguous", xd),)


def _reference(x, what, b):
    """{(dtype, with_bias): device tensor} of the exact Y over all rows of x, and the float64 Y itself on the device: float32 holds
    the float64 product exactly (asserted), bf16 is torch's round-to-nearest-even of that float32 on the host."""
    b64 = b.astype(np.float64)
    _grid_preconditions(x, what, b64)
    out = {}
    for with_bias in (False, True):
        want = x.astype(np.float64) @ what.T + (b64[None, :] if with_bias else 0.0) + 0.0      # + 0.0: a zero sum is +0, as an accumulator
        want32 = want.astype(np.float32)                                                    # that starts at +0 leaves it
        assert np.array_equal(want32.astype(np.float64), want)
        t32 = torch.from_numpy(want32)
        out[torch.float32, with_bias] = t32.cuda()
        out[torch.bfloat16, with_bias] = t32.to(torch.bfloat16).cuda()
        out["float64", with_bias] = torch.from_numpy(want).cuda()
    return out


@functools.lru_cache(maxsize=None)
def _weight(n, k, which):
    """(packed W(n, k) on the device, Ŵ float64, bias float32 on the host, bias on the device, the references over the 256 rows of
    _x(k)) — packed once per (n, k, map), never written to."""
    _x0, w, b = _grid_case(1, n, k, 1000 * n + k)
    amap = _map(n, k, which)
    what = _what(w, amap)
    pt = packed.pack(w, amap, backend="hip")
    return pt, w, amap, torch.from_numpy(b).cuda(), _reference(_x(k)[0], what, b)


def _check_y(got, ref, dtype, with_bias, m, what):
    """got (m, n) of `dtype` against the references' first m rows: the float64 product as values, the bf16 rounding as bits."""
    if dtype == torch.float32:
        _must_equal(got.double(), ref["float64", with_bias][:m], what)
    else:
        _must_equal(_ints(got), _ints(ref[dtype, with_bias][:m]), what)


# ----------------------------------------------------------------------------- block and wide

@pytest.mark.parametrize("k", KS)
def test_block_and_wide_equal_the_float64_product(k):
    for n in NS:
        for which in WHICH:
            pt, _w, _amap, bd, ref = _weight(n, k, which)
            tables = pt.tables()
            for layout, xd in _layouts(k):
                for m in MS:
                    for dtype in DTYPES:
                        for with_bias in (False, True):
                            what = (m, n, k, which, layout, dtype, with_bias)
                            bias = bd if with_bias else None
                            block = hb.packed_linear(xd[:m], pt.data, tables, n, bias=bias, out_dtype=dtype)
                            wide = hb.packed_linear_wide(xd[:m], pt.data, tables, n, bias=bias, out_dtype=dtype)
                            _check_y(block, ref, dtype, with_bias, m, ("block",) + what)
                            _check_y(wide, ref, dtype, with_bias, m, ("wide",) + what)
                            _must_equal(_ints(wide), _ints(block), ("wide has the block kernel's bits",) + what)


# ----------------------------------------------------------------------------- skinny

def _library_split(m, n, k):
    """The effective split of split = 0.  The workspace is split · m · n floats rounded up to 16 bytes, which names the split only from
    16 bytes up: it is read at m = 32 (the split is a function of the shape's tile grid) and must then give the workspace of (m, n, k)."""
    eff = max(1, hb.packed_linear_skinny_workspace_bytes(32, n, k, 0) // (4 * 32 * n))
    assert hb.packed_linear_skinny_workspace_bytes(m, n, k, eff) == hb.packed_linear_skinny_workspace_bytes(m, n, k, 0), (m, n, k, eff)
    return eff


@pytest.mark.parametrize("k", KS)
def test_skinny_equals_the_float64_product_at_every_split(k):
    tiles_w = orc.tiles_hw(1, k)[1]
    for n in NS:
        for which in WHICH:
            pt, _w, _amap, bd, ref = _weight(n, k, which)
            tables = pt.tables()
            for layout, xd in _layouts(k):
                for m in (m for m in MS if m <= hb.PACKED_SKINNY_MAX_M):
                    eff = _library_split(m, n, k)
                    assert 1 <= eff <= tiles_w
                    for dtype in DTYPES:
                        for with_bias in (False, True):
                            bias = bd if with_bias else None
                            got = {}
                            for split in dict.fromkeys((0, 1, 2, tiles_w + 1, eff)):
                                what = ("skinny", m, n, k, which, layout, dtype, with_bias, split)
                                got[split] = hb.packed_linear_skinny(xd[:m], pt.data, tables, n, bias=bias, out_dtype=dtype, split=split)
                                _check_y(got[split], ref, dtype, with_bias, m, what)
                            _must_equal(_ints(got[0]), _ints(got[eff]), ("split 0 is the library's split", m, n, k, which, layout, dtype, with_bias, eff))


# ----------------------------------------------------------------------------- grouped

@functools.lru_cache(maxsize=None)
def _experts(n, k):
    """Three experts of (n, k) in one arena: random maps with different seeds around a uniform bfp4 one."""
    ws, bs, maps = [], [], []
    for e in range(3):
        _x0, w, b = _grid_case(1, n, k, 50000 + 1000 * n + 10 * k + e)
        ws.append(w)
        bs.append(b)
        maps.append(_map(n, k, ("random", "bfp4", "random")[e], seed=17 * e))
    w3, b3, maps = np.stack(ws), np.stack(bs), np.stack(maps)
    pts = packed.pack_batch(torch.from_numpy(w3).cuda(), maps, backend="hip")
    x = _x(k)[0][:GROUPED_T]
    refs = [_reference(x, _what(w3[e], maps[e]), b3[e]) for e in range(3)]
    return packed.batch_of(pts), torch.from_numpy(b3).cuda(), refs


@pytest.mark.parametrize("k", GROUPED_KS)
def test_grouped_equals_the_float64_product_per_expert(k):
    assert set(sum(GROUPED_ROWS, ())) == {0, 1, 31, 32, 33, 65}
    assert GROUPED_ROWS[0][0] == GROUPED_ROWS[0][1] and GROUPED_ROWS[1][2] == GROUPED_ROWS[1][3]      # an empty group first, and last
    for n in GROUPED_NS:
        batch, bd, refs = _experts(n, k)
        for layout, xd in _layouts(k):
            for rows in GROUPED_ROWS:
                rows_dev = torch.tensor(rows, dtype=torch.int32, device="cuda")
                for dtype in DTYPES:
                    for with_bias in (False, True):
                        for split in (0, 2):
                            what = ("grouped", n, k, layout, rows, dtype, with_bias, split)
                            y = hb.packed_linear_skinny_grouped(xd[:GROUPED_T], rows_dev, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev,
                                                                3, n, bias=bd if with_bias else None, out_dtype=dtype, split=split)
                            assert tuple(y.shape) == (GROUPED_T, n) and y.dtype == dtype
                            covered = torch.zeros(GROUPED_T, dtype=torch.bool, device="cuda")
                            for e in range(3):
                                r0, r1 = rows[e], rows[e + 1]
                                covered[r0:r1] = True
                                if dtype == torch.float32:
                                    _must_equal(y[r0:r1].double(), refs[e]["float64", with_bias][r0:r1], what + (e,))
                                else:
                                    _must_equal(_ints(y[r0:r1]), _ints(refs[e][dtype, with_bias][r0:r1]), what + (e,))
                            assert not bool(y[~covered].any()), what + ("rows of no group are the zeros the entry allocated",)


# ----------------------------------------------------------------------------- unpack

@pytest.mark.parametrize("k", KS)
def test_unpack_is_the_oracles_reconstruction_inside_a_frame(k):
    for n in NS:
        for which in WHICH:
            pt, w, amap, _bd, _ref = _weight(n, k, which)
            want = expected_bits(w, amap)
            assert want.shape == (n, k) and np.all(want & np.uint32(0xFFFF) == 0)                  # every format's values are bf16-valued
            want32 = torch.from_numpy(want.view(np.int32)).cuda()
            want16 = torch.from_numpy((want >> np.uint32(16)).astype(np.uint16).view(np.int16)).cuda()
            for dtype in DTYPES:
                # an odd first column: element stores; column 8 of a pitch that is a multiple of 8: rows on 16-byte addresses
                for c0, pitch in ((3, k + 7), (8, (k + 23) // 8 * 8)):
                    buf = torch.full((n + 2, pitch), SENTINEL, dtype=dtype, device="cuda")
                    out = buf[1:1 + n, c0:c0 + k]
                    assert (out.data_ptr() % 16 == 0 and (pitch * buf.element_size()) % 16 == 0) == (c0 == 8)
                    got = hb.unpack_tiles(pt.data, pt.tables(), n, k, dtype=dtype, out=out)
                    assert got.data_ptr() == out.data_ptr()
                    _must_equal(_ints(out.contiguous()), want32 if dtype == torch.float32 else want16, ("unpack", n, k, which, dtype, c0))
                    frame = torch.ones_like(buf, dtype=torch.bool)
                    frame[1:1 + n, c0:c0 + k] = False
                    assert bool((buf[frame] == SENTINEL).all()), ("the frame was written", n, k, which, dtype, c0)


# ----------------------------------------------------------------------------- specials: the wide kernel is the block kernel

def _must_be_same_nan_aware(got, want, what):
    gn, wn = torch.isnan(got), torch.isnan(want)
    _must_equal(gn, wn, what + ("NaN positions",))
    zero = torch.zeros((), dtype=_ints(got).dtype, device=got.device)
    _must_equal(torch.where(gn, zero, _ints(got)), torch.where(wn, zero, _ints(want)), what)


@pytest.mark.parametrize("k", [1, 8, 32, 64, 128, 256, 384])
def test_wide_is_the_block_kernel_on_specials(k):
    xh = to_bf16_valued(gen("normal_f32", 61 + k, (129, k)) * 40)
    xd = torch.from_numpy(xh).to(torch.bfloat16).cuda()
    buf = torch.zeros((129, k + 9), dtype=torch.bfloat16, device="cuda")
    buf[:, 1:1 + k] = xd
    for n in (1, 64, 128, 129):
        bd = torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda()
        for which in WHICH:
            pt = packed.pack(specials((n, k), seed=n + k), _map(n, k, which), backend="hip")
            for layout, x in (("contiguous", xd), ("pitched", buf[:, 1:1 + k])):
                for m in (1, 64, 128, 129):
                    for dtype in DTYPES:
                        for bias in (None, bd):
                            what = ("specials", m, n, k, which, layout, dtype, bias is not None)
                            block = hb.packed_linear(x[:m], pt.data, pt.tables(), n, bias=bias, out_dtype=dtype)
                            wide = hb.packed_linear_wide(x[:m], pt.data, pt.tables(), n, bias=bias, out_dtype=dtype)
                            _must_be_same_nan_aware(wide, block, what)


# ----------------------------------------------------------------------------- one-hot

# (n, k = m, s, the tile whose byte is flipped, row and column in the tile): one K step and whole blocks; four steps, the flipped tile in
# the last step's tile column (columns 192..255 are tile columns 6 and 7) and in the one-row tile row of the second N block
ONE_HOT = [(128, 64, 3, (3, 1), 3, 5), (129, 256, -2, (4, 7), 0, 5)]


@pytest.mark.parametrize("n,k,s,tile,row,col", ONE_HOT)
def test_one_hot_pins_every_position_and_a_flipped_byte(n, k, s, tile, row, col):
    """tests/test_packed_wide_gpu.py's test_wide_one_hot_pins_every_position at these shapes, through the wide and the block kernel."""
    w = gen("heavy_f32", 50 + n, (n, k))
    amap = random_map((n, k), 51 + n).copy()
    amap[tile] = 1                                   # bfp8: one code per byte
    want = (2.0 ** s) * _what(w, amap).T
    assert want.shape == (k, n) and np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    eye = np.eye(k, dtype=np.float32) * np.float32(2.0 ** s)
    assert np.array_equal(to_bf16_valued(eye), eye)
    xd = torch.from_numpy(eye).to(torch.bfloat16).cuda()
    pt = packed.pack(w, amap, backend="hip")
    tr, tc = tile
    steps = -(-k // 64)
    assert 32 * tr + row < n and 64 * (steps - 1) <= 32 * tc + col < k
    t = tr * amap.shape[1] + tc
    for flipped in (False, True):
        if flipped:                                  # element (row, col) of the tile changes its last mantissa bit
            pt.data[int(pt.offsets[t]) * 64 + 64 + 32 * row + col] ^= 0x01
        for name, entry in (("wide", hb.packed_linear_wide), ("block", hb.packed_linear)):
            y = entry(xd, pt.data, pt.tables(), n).cpu().numpy().astype(np.float64)
            bad = [tuple(r) for r in np.argwhere(y != want)]
            assert bad == ([(32 * tc + col, 32 * tr + row)] if flipped else []), (name, flipped, bad[:8])      # Y[k, n] alone


def test_the_lattice_reaches_the_step_counts_and_blocks_it_is_there_for():
    assert sorted({-(-k // 64) for k in KS}) == [1, 2, 3, 4, 6]
    assert {k for k in KS if k <= 32} == {1, 7, 8, 9, 16, 17, 31, 32} and set(PITCHED_KS) >= {1, 7, 33, 8, 64, 128, 192, 256, 384}
    assert {64, 128, 256} <= set(NS) and {128, 256} <= set(MS) and 1 in NS and 1 in MS
    assert set(GROUPED_KS) <= set(KS) and GRID == 2.0 ** -8 and 4 * max(KS) * 256 + 255 < 2 ** 19
