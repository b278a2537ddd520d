"""GPU: the wide-block packed linear (packed_wide_kernel<.., WT = false>, csrc/mtq_packed.hip) held to its bit contract — for every input the
block kernel's output bit for bit — and, independently of the block kernel, to exact arithmetic and to the oracle's Ŵ.

The block is 128 (M) × 128 (N) × 64 (K), four waves 2 × 2 of 64 × 64 outputs.  The shapes:

  m = 1, 33     one row block, almost empty; 33 is a second 32-row MFMA block of one row;
  m = 257       a third row block of one row, with whole wave sub-blocks past m;
  m = 300       three row blocks, ragged inside a 32-row MFMA block (300 = 9·32 + 12);
  n = 72        one N block, its third tile row ragged (8 of 32), the wave of the fourth tile row without tiles;
  n = 200       a second N block, ragged in its third tile row (200 = 6·32 + 8): 7 tile rows;
  k = 100       two K steps, the last tile column ragged inside a group (100 = 3·32 + 4): the second step is the last, staged in the loop;
  k = 300       five steps (both register sets and both LDS images several times, an odd count), ten tile columns, the last ragged;
  k = 2100      33 steps, 66 tile columns, once at (300, 200);
  k = 104, 320  a contiguous X with k % 8 == 0 is read by 16-byte loads (every other X here, the pitched one included, element by
                element): two steps with a ragged last tile column (104 = 3·32 + 8), and five whole steps.

Maps: random over all four codes, and all-bfp4.

  * bit contract: heavy-tailed float32 weights and bf16 X: float32 and bf16 Y, with and without bias, X contiguous (vector loads) and at
    a pitch with an unaligned first element (scalar loads), Y into a pitched buffer whose sentinels stay, every call twice; the same
    over the specials tensor (Inf, NaN, denormals, exponent bytes 0 and 255): NaN exactly where the block kernel has NaN, equal bits
    everywhere else;
  * integer grid (tests/test_packed_gpu.py's construction and preconditions: every order is exact): Y EQUALS the float64 product;
  * one-hot: X = 2ˢ·I, m = k = 300 in one call: every (n, k) position is the oracle's Ŵ; one flipped code byte shows at its position;
  * guards: packed_bytes cut short of the last tile and map codes 4 and −1, over buffers that stay whole: zeros for that tile;
  * routing: auto at m = 300 is the block kernel's bits whatever the gate; m = 0.
"""
from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import GRID, TILE_BYTES, _grid_case, _grid_preconditions, expected_bits, random_map, specials, uniform_map

pytestmark = pytest.mark.gpu
SHAPES = [(m, n, k) for m in (1, 33, 257, 300) for n in (72, 200) for k in (100, 300)] + [(300, 200, 2100)]
SHAPES += [(1, 72, 320), (33, 200, 104), (257, 72, 104), (300, 200, 320)]       # k % 8 == 0: the kernel's 16-byte loads of X
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def _what(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """Ŵ as float64, from the oracle."""
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _bits(t) -> np.ndarray:
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _maps(n, k):
    return (("random", random_map((n, k), n + k)), ("bfp4", uniform_map((n, k), 2)))


@functools.lru_cache(maxsize=None)
def _weight(n, k, kind, which):
    """The packed weight of (n, k) on the device and its bias — made once per (n, k, values, map), never written to."""
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", 7 * n + k, (n, k))
    amap = dict(_maps(n, k))[which]
    return packed.pack(w, amap, backend="hip"), torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda()


@functools.lru_cache(maxsize=None)
def _x(m, k):
    x = _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 40))
    pitched = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    pitched[:, 1:1 + k] = x
    view = pitched[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and (m == 1 or view.stride(0) % 8 != 0)   # the scalar load path
    return x, view


def _wide_into_sentinels(xd, pt, n, bias, dtype):
    """hb.packed_linear_wide into a pitched view of a buffer of sentinels → the (m, n) result; the columns and rows around it stay."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_linear_wide(xd, pt.data, pt.tables(), n, bias=bias, out_dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = buf.float().cpu().numpy()
    inside = np.zeros(whole.shape, dtype=bool)
    inside[1:1 + m, 2:2 + n] = True
    assert np.all(whole[~inside] == sentinel), (m, n, np.argwhere((whole != sentinel) & ~inside)[:4])
    return out


def _same(got, want, nan_aware, what):
    g, w = _bits(got), _bits(want)
    if nan_aware:
        gn, wn = torch.isnan(got).cpu().numpy(), torch.isnan(want).cpu().numpy()
        assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:4])
        g, w = np.where(gn, 0, g), np.where(wn, 0, w)
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:4])


def _bit_contract(m, n, k, kind):
    plain, pitched = _x(m, k)
    for which, _amap in _maps(n, k):
        pt, bd = _weight(n, k, kind, which)
        for layout, xd in (("contiguous", plain), ("pitched", pitched)):
            for out_dtype, dtype in DTYPES:
                for bias in (None, bd):
                    what = (m, n, k, kind, which, layout, out_dtype, bias is not None)
                    block = packed.linear(xd, pt, bias=bias, out_dtype=out_dtype, kernel="block")
                    assert tuple(block.shape) == (m, n) and block.dtype == dtype
                    y = packed.linear_wide(xd, pt, bias=bias, out_dtype=out_dtype)
                    assert tuple(y.shape) == (m, n) and y.dtype == dtype
                    _same(y, block, kind == "specials", what)
                    assert np.array_equal(_bits(packed.linear_wide(xd, pt, bias=bias, out_dtype=out_dtype)), _bits(y)), what
                    first = _wide_into_sentinels(xd, pt, n, bias, dtype)
                    _same(first, block, kind == "specials", what)
                    again = _wide_into_sentinels(xd, pt, n, bias, dtype)
                    assert np.array_equal(_bits(again.contiguous()), _bits(first.contiguous())), what


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_wide_is_the_block_kernel_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy")


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_wide_is_the_block_kernel_on_specials(m, n, k):
    _bit_contract(m, n, k, "specials")


# ----------------------------------------------------------------------------- independent of the block kernel

@pytest.mark.parametrize("m,n,k", [(300, 200, 300), (257, 72, 2100), (300, 200, 320)])
def test_wide_integer_grid_is_exact(m, n, k):
    x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
    xd, bd = _x_dev(x), torch.from_numpy(b).cuda()
    b64 = b.astype(np.float64)
    for which, amap in _maps(n, k):
        what = _what(w, amap)
        _grid_preconditions(x, what, b64)
        want = x.astype(np.float64) @ what.T + b64[None, :]
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        want_bf16 = torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)
        pt = packed.pack(w, amap, backend="hip")
        got = hb.packed_linear_wide(xd, pt.data, pt.tables(), n, bias=bd).cpu().numpy()
        assert got.shape == (m, n) and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want), (m, n, k, which, np.argwhere(got != want)[:4])
        nob = hb.packed_linear_wide(xd, pt.data, pt.tables(), n).cpu().numpy()
        assert np.array_equal(nob.astype(np.float64), want - b64[None, :]), (m, n, k, which)
        yb = hb.packed_linear_wide(xd, pt.data, pt.tables(), n, bias=bd, out_dtype=torch.bfloat16)
        assert np.array_equal(_bits(yb), _bits(want_bf16)), (m, n, k, which)


ONE_HOT = (200, 300, 3)                              # n, k = m, s
FLIP_TILE, FLIP_ROW, FLIP_COL = (5, 6), 3, 5         # a tile of the second N block (tile rows 4..6) and the fourth K step (columns 192..255)


@functools.lru_cache(maxsize=None)
def _one_hot():
    n, k, s = ONE_HOT
    w = gen("heavy_f32", 50 + n, (n, k))
    amap = random_map((n, k), 51 + n).copy()
    amap[FLIP_TILE] = 1                              # bfp8: one code per byte
    want = (2.0 ** s) * _what(w, amap).T
    assert want.shape == (k, n) and np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return w, amap, want, _x_dev(np.eye(k, dtype=np.float32) * np.float32(2.0 ** s))


def test_wide_one_hot_pins_every_position():
    w, amap, want, xd = _one_hot()
    n = ONE_HOT[0]
    pt = packed.pack(w, amap, backend="hip")
    y = hb.packed_linear_wide(xd, pt.data, pt.tables(), n).cpu().numpy().astype(np.float64)
    bad = np.argwhere(y != want)
    assert bad.size == 0, bad[:8]
    # one code byte of the chosen tile: element (FLIP_ROW, FLIP_COL) changes its last mantissa bit
    tr, tc = FLIP_TILE
    assert 128 <= 32 * tr < n and 3 * 64 <= 32 * tc < 4 * 64
    t = tr * amap.shape[1] + tc
    pt.data[int(pt.offsets[t]) * 64 + 64 + 32 * FLIP_ROW + FLIP_COL] ^= 0x01
    y = hb.packed_linear_wide(xd, pt.data, pt.tables(), n).cpu().numpy().astype(np.float64)
    assert [tuple(r) for r in np.argwhere(y != want)] == [(32 * tc + FLIP_COL, 32 * tr + FLIP_ROW)]      # Y[k, n] alone


# ----------------------------------------------------------------------------- blobs that are not there

def _zeroed(what, tiles_w, tiles):
    out = what.copy()
    for t in tiles:
        tr, tc = divmod(int(t), tiles_w)
        out[32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 300, 200, 300
    x, w, b = _grid_case(m, n, k, 77)
    amap = random_map((n, k), 78)
    what = _what(w, amap)
    _grid_preconditions(x, what, b.astype(np.float64))
    return n, packed.pack(w, amap, backend="hip"), what, b, x


def _guarded(tables, gone):
    """Through `tables`: the block kernel's bits, and the float64 product with the tiles `gone` as zeros.  pt.data is the whole stream:
    a kernel without the guard reads real bytes and the comparison fails."""
    n, pt, what, b, x = _guard_case()
    assert pt.data.numel() == pt.nbytes == pt.tables().nbytes                # never a shorter buffer
    what_left = _zeroed(what, pt.map.shape[1], gone)
    assert np.count_nonzero(what_left != what) > 0
    xd, bd = _x_dev(x), torch.from_numpy(b.copy()).cuda()
    for bias in (None, bd):
        want = x.astype(np.float64) @ what_left.T + (0.0 if bias is None else b.astype(np.float64)[None, :])
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        for dtype in (torch.float32, torch.bfloat16):
            block = hb.packed_linear(xd, pt.data, tables, n, bias=bias, out_dtype=dtype)
            y = hb.packed_linear_wide(xd, pt.data, tables, n, bias=bias, out_dtype=dtype)
            assert np.array_equal(_bits(y), _bits(block)), (dtype, bias is not None)
            if dtype == torch.float32:
                g = y.cpu().numpy().astype(np.float64)
                assert np.array_equal(g, want), (bias is not None, np.argwhere(g != want)[:4])


def test_wide_reads_a_blob_past_packed_bytes_as_zeros():
    n, pt, what, b, x = _guard_case()
    tiles = pt.map.size
    last = tiles - 1
    cut = int(pt.offsets[last]) * 64 + TILE_BYTES[int(pt.map.reshape(-1)[last])] - 64      # 64 bytes short of the end of the last tile
    assert tiles * TILE_BYTES[3] <= cut < pt.nbytes                          # the entries refuse less
    short = copy.copy(pt.tables())                                           # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    _guarded(short, (last,))
    assert pt.tables().nbytes == pt.nbytes                                   # the shared tables were not touched


def test_wide_reads_a_tile_whose_map_code_is_no_format_as_zeros():
    n, pt, what, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    tables = hb.PackedTables.on_device(pt.map, pt.offsets)                   # a private copy
    inner = (1 * tiles_w + 3, 5 * tiles_w + 6)                               # first N block, second K step; second N block, fourth K step
    assert all(0 < t // tiles_w < tiles_h - 1 and 0 < t % tiles_w < tiles_w - 1 for t in inner)
    tables.map_dev[inner[0]] = 4
    tables.map_dev[inner[1]] = -1
    _guarded(tables, inner)
    assert np.array_equal(pt.tables().map_dev.cpu().numpy(), pt.map.reshape(-1))


# ----------------------------------------------------------------------------- routing

def test_auto_at_m_300_is_the_block_kernels_bits_and_m_0_is_empty():
    m, n, k = 300, 200, 300
    plain, _pitched = _x(m, k)
    pt, bd = _weight(n, k, "heavy", "random")
    for out_dtype, dtype in DTYPES:
        block = packed.linear(plain, pt, bias=bd, out_dtype=out_dtype, kernel="block")
        assert np.array_equal(_bits(packed.linear(plain, pt, bias=bd, out_dtype=out_dtype, kernel="auto")), _bits(block))
        layer = packed.PackedLinear(pt, bias=bd, out_dtype=out_dtype)
        assert layer.kernel == "auto" and layer.backend == "hip"
        assert np.array_equal(_bits(layer(plain)), _bits(block))
        assert np.array_equal(_bits(layer(plain.reshape(3, 100, k)).reshape(m, n)), _bits(block))
        empty = packed.linear_wide(plain[:0], pt, bias=bd, out_dtype=out_dtype)
        assert tuple(empty.shape) == (0, n) and empty.dtype == dtype and empty.is_cuda
