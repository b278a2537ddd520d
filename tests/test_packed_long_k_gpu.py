"""GPU: the two packed linear kernels at rows long enough to reach the code that tests/test_packed_gpu.py and
tests/test_packed_skinny_gpu.py (k <= 200, at most 7 tile columns) never run, held to the same references: Ŵ from the oracle, Y from the
float64 product on the host.  n = 70 (3 tile rows, the last ragged) unless said otherwise; each k is there for a branch:

  k = 288   9 tile columns: the skinny kernel's ring of kSkinnyRing = 8 tiles takes a second round, holding one tile; the library's own
            split is 2, with uneven slices of 4 and 5 tiles;
  k = 300   10 tile columns, the last ragged (12 of 32 positions);
  k = 520   17 tile columns: three ring rounds, the last partial;
  k = 2100  66 tile columns, the last ragged: a second 64-tile chunk of map and offsets, holding two tiles; the library's split is 16;
  k = 4200  132 tile columns: at split 2 both slices run into a second chunk and the second starts at c0 = 66; the library's split is 33;
  n = 19200, k = 512, m = 32   600 tile rows: the units side of the split rule decides (3 slices of 5, 5 and 6 tiles over 16 columns),
            450 workgroups.
At every shape the splits include tiles_w (one tile per slice) and tiles_w + 3 (clamped to tiles_w).  The block kernel walks the same
rows: up to 66 K steps of 64, `locate` two steps ahead over mixed blobs.

  * integer grid (grid_case_is_exact of test_packed_skinny_gpu.py, preconditions asserted per case): Y EQUALS the float64 product with and
    without bias, the bf16 Y is the once-rounded float32 Y, skinny and block agree bit for bit; the block kernel also at m = 133;
  * the library's split, recovered from the workspace size, is above 1 at every shape and split = 0 gives that split's bits;
  * one-hot: X = rows [32c, 32c + 32) of 2ˢ·I_k: the assembled k × n result is 2ˢ·Ŵᵀ at every position, at split 1, the library's split
    and 2, and from the block kernel with m = k; a flipped code byte in a tile of the second ring round, and of the second chunk, shows
    at exactly its position;
  * random (random_case_is_within_the_bound of test_packed_skinny_gpu.py): the (k + 2)·2⁻²⁴·(Σ|x||ŵ| + |b|) bound at long K, both X
    layouts, the workspace's contents, a pitched Y;
  * PackedLinear with a workspace that exists: calls with m = 1, 32, 5, 1 on one instance are packed.linear's bits on a fresh workspace
    (and within the bound of the float64 product); m = 33 is the block kernel;
  * blobs that are not there read as zeros in both kernels: packed_bytes cut short of a tile (the stream buffer stays whole), and map
    codes 4 and −1 in the first and the second ring round.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import TILE_BYTES, _grid_preconditions, random_map
from tests.test_packed_skinny_gpu import _bits, _grid_weight, _what, _x_dev, grid_case_is_exact, random_case_is_within_the_bound

pytestmark = pytest.mark.gpu

LONG_KS = (288, 300, 520, 2100, 4200)
BIG = (19200, 512)                                   # (n, k): 600 tile rows
SHAPES = [(70, k) for k in LONG_KS] + [BIG]


def _splits(k):
    tiles_w = orc.tiles_hw(1, k)[1]
    return (0, 1, 2, 5, tiles_w, tiles_w + 3)


def _library_split(m, n, k):
    """The effective split of split = 0, from the workspace it asks for (a host function): split · m · n floats, rounded up to 16 bytes."""
    assert 4 * m * n >= 16
    return hb.packed_linear_skinny_workspace_bytes(m, n, k, 0) // (4 * m * n)


# ----------------------------------------------------------------------------- integer grid

@pytest.mark.parametrize("m", [1, 17, 32])
@pytest.mark.parametrize("k", LONG_KS)
def test_long_k_integer_grid_is_exact(k, m):
    assert orc.tiles_hw(70, k)[1] > 8                                       # a second ring round at split 1
    grid_case_is_exact(m, 70, k, splits=_splits(k))


def test_many_tile_rows_integer_grid_is_exact():
    n, k = BIG
    assert orc.tiles_hw(n, k) == (600, 16)
    grid_case_is_exact(32, n, k, splits=_splits(k))


def test_block_kernel_long_k_integer_grid_is_exact_at_m_133():
    m, n, k = 133, 70, 2100
    x = np.random.default_rng(1000 * m + 10 * n + k).integers(-4, 5, size=(m, k)).astype(np.float32)
    xd = _x_dev(x)
    for which in ("random", "0", "1", "2", "3"):
        pt, what, b = _grid_weight(n, k, which)
        b64 = b.astype(np.float64)
        _grid_preconditions(x, what, b64)
        want = x.astype(np.float64) @ what.T + b64[None, :]
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        bd = torch.from_numpy(b.copy()).cuda()
        got = packed.linear(xd, pt, bias=bd).cpu().numpy()
        assert got.shape == (m, n) and np.array_equal(got.astype(np.float64), want), (which, np.argwhere(got != want)[:4])
        nob = packed.linear(xd, pt).cpu().numpy()
        assert np.array_equal(nob.astype(np.float64), want - b64[None, :]), which
        yb = packed.linear(xd, pt, bias=bd, out_dtype="bfloat16")
        assert np.array_equal(_bits(yb), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))), which


# ----------------------------------------------------------------------------- the library's own split

@pytest.mark.parametrize("n,k", SHAPES)
def test_the_librarys_split_is_above_one_and_is_what_split_0_runs(n, k):
    pt, what, b = _grid_weight(n, k, "random")
    bd = torch.from_numpy(b.copy()).cuda()
    for m in ((1, 17, 32) if n == 70 else (32,)):
        split = _library_split(m, n, k)
        print(f"n={n} k={k} m={m}: the library's split is {split}")
        assert split > 1
        assert hb.packed_linear_skinny_workspace_bytes(m, n, k, split) == hb.packed_linear_skinny_workspace_bytes(m, n, k, 0)
        x = np.random.default_rng(7 * m + n + k).integers(-4, 5, size=(m, k)).astype(np.float32)
        _grid_preconditions(x, what, b.astype(np.float64))
        xd = _x_dev(x)
        for out_dtype in ("float32", "bfloat16"):
            explicit = packed.linear(xd, pt, bias=bd, kernel="skinny", split=split, out_dtype=out_dtype)
            direct = packed.linear(xd, pt, bias=bd, kernel="skinny", split=1, out_dtype=out_dtype)
            for got in (packed.linear(xd, pt, bias=bd, kernel="skinny", split=0, out_dtype=out_dtype),
                        packed.linear(xd, pt, bias=bd, kernel="skinny", out_dtype=out_dtype),
                        packed.linear(xd, pt, bias=bd, kernel="auto", out_dtype=out_dtype)):
                assert np.array_equal(_bits(got), _bits(explicit)), (m, n, k, out_dtype)
            assert np.array_equal(_bits(direct), _bits(explicit)), (m, n, k, out_dtype)          # the integer grid: every order is exact


# ----------------------------------------------------------------------------- one-hot

def _code_byte(pt, tr, tc, r, c):
    """(byte index in the stream, bit mask) of the lowest mantissa bit of element (r, c) of tile (tr, tc), from pt.offsets and the
    format's layout: a bf16 blob is 1024 little-endian uint16 in row-major order e = 32 r + c; a BFP blob is 64 exponent bytes and then
    the codes (sign << M) | man, one per byte (bfp8), two per byte with even e in the low nibble (bfp4), four per byte with e at bits
    2 (e % 4) (bfp2)."""
    tiles_w = pt.map.shape[1]
    f = int(pt.map[tr, tc])
    base = int(pt.offsets[tr * tiles_w + tc]) * 64
    e = 32 * r + c
    if f == 0:
        return base + 2 * e, 0x01
    if f == 1:
        return base + 64 + e, 0x01
    if f == 2:
        return base + 64 + e // 2, 0x01 << (4 * (e % 2))
    return base + 64 + e // 4, 0x01 << (2 * (e % 4))


def _one_hot_case(n, k, s, seed, flip=None):
    """(packed weight, 2ˢ·Ŵᵀ float64 (k, n), 2ˢ·I_k float32).  flip = (tr, tc, r, c): that element's lowest mantissa bit is flipped in
    the stream, not in Ŵ."""
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((n, k), seed + 1).copy()
    amap[0, 0] = 1
    pt = packed.pack(w, amap, backend="hip")
    if flip is not None:
        at, mask = _code_byte(pt, *flip)
        assert 0 <= at < pt.nbytes
        pt.data[at] ^= mask
    eye = np.eye(k, dtype=np.float32) * np.float32(2.0 ** s)
    want = (2.0 ** s) * _what(w, amap).T
    assert want.shape == (k, n)
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return pt, want, eye


def _one_hot_mismatches(pt, want, eye, split):
    """split None: the block kernel on the whole 2ˢ·I_k (m = k); otherwise the skinny kernel, 32 rows of it per call."""
    k = eye.shape[0]
    if split is None:
        y = packed.linear(_x_dev(eye), pt)
    else:
        y = torch.cat([packed.linear(_x_dev(eye[c:c + 32]), pt, kernel="skinny", split=split) for c in range(0, k, 32)])
    y = y.cpu().numpy().astype(np.float64)
    assert y.shape == want.shape
    return np.argwhere(y != want)


def _one_hot_routes(n, k):
    lib = _library_split(32, n, k)
    assert lib > 1
    return tuple(dict.fromkeys((1, lib, 2, None)))


@pytest.mark.parametrize("n,k,s", [(70, 300, 3), (70, 2100, -2)])
def test_long_k_one_hot_pins_every_position(n, k, s):
    pt, want, eye = _one_hot_case(n, k, s, 50 + k)
    for split in _one_hot_routes(n, k):
        bad = _one_hot_mismatches(pt, want, eye, split)
        assert bad.size == 0, (split, bad[:8])


# (n, k, flipped element (tile row, tile column, row, column)): tile column 8 or later is of the second ring round at split 1, 64 or
# later of the second chunk; (2, 9) and (2, 65) are ragged in both directions
@pytest.mark.parametrize("n,k,flip", [(70, 300, (1, 8, 3, 5)), (70, 300, (2, 9, 4, 11)), (70, 2100, (0, 12, 31, 31)), (70, 2100, (1, 64, 17, 0)),
                                      (70, 2100, (2, 65, 5, 19))])
def test_long_k_one_hot_fails_on_a_wrong_image(n, k, flip):
    tr, tc, r, c = flip
    assert tc >= 8 and 32 * tr + r < n and 32 * tc + c < k
    pt, want, eye = _one_hot_case(n, k, 3, 120 + k, flip=flip)
    for split in _one_hot_routes(n, k):
        bad = _one_hot_mismatches(pt, want, eye, split)
        assert [tuple(x) for x in bad] == [(32 * tc + c, 32 * tr + r)], (split, bad[:8])         # Y[k, n] of that element alone


# ----------------------------------------------------------------------------- random values

@pytest.mark.parametrize("m,n,k", [(1, 70, 300), (17, 130, 2100), (32, 70, 4200)])
def test_long_k_random_is_within_the_f32_accumulation_bound(m, n, k):
    assert _library_split(m, n, k) > 1                                      # split 0 is a split route here
    random_case_is_within_the_bound(m, n, k)


# ----------------------------------------------------------------------------- PackedLinear

@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("k", [288, 2100])
def test_packed_linear_module_keeps_a_real_workspace(k, out_dtype):
    n = 70
    w = gen("heavy_f32", 80 + k, (n, k))
    amap = random_map((n, k), 81 + k)
    pt = packed.pack(w, amap, backend="hip")
    b = gen("normal_f32", 82 + k, (n,))
    bd = torch.from_numpy(b).cuda()
    xh = to_bf16_valued(gen("normal_f32", 83 + k, (33, k)))
    x33 = _x_dev(xh)
    what = _what(w, amap)
    want = xh.astype(np.float64) @ what.T + b.astype(np.float64)[None, :]
    bound = (k + 2) * 2.0 ** -24 * (np.abs(xh).astype(np.float64) @ np.abs(what).T + np.abs(b).astype(np.float64)[None, :])
    if out_dtype == "bfloat16":                      # one more rounding, relative 2⁻⁸
        bound = bound * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want)
    layer = packed.PackedLinear(pt, bias=bd, out_dtype=out_dtype)
    assert layer.backend == "hip" and layer.kernel == "auto"
    need = max(hb.packed_linear_skinny_workspace_bytes(m, n, k) for m in range(1, 33))
    assert need > 0 and layer._workspace is not None and layer._workspace.numel() >= need
    first = {}
    for m in (1, 32, 5, 1):                          # a larger partial layout over a smaller one's and back, in one kept workspace
        assert _library_split(m, n, k) > 1
        x = x33[:m]
        y = layer(x)
        assert tuple(y.shape) == (m, n) and y.is_cuda and y.dtype == (torch.float32 if out_dtype == "float32" else torch.bfloat16)
        fresh = packed.linear(x, pt, bias=bd, out_dtype=out_dtype, kernel="auto")
        assert np.array_equal(_bits(y), _bits(fresh)), (k, out_dtype, m)
        assert np.array_equal(_bits(y), _bits(packed.linear(x, pt, bias=bd, out_dtype=out_dtype, kernel="skinny"))), (k, out_dtype, m)
        assert np.array_equal(first.setdefault(m, _bits(y)), _bits(y)), (k, out_dtype, m)         # m = 1 again: the same bits
        assert np.all(np.abs(y.float().cpu().numpy().astype(np.float64) - want[:m]) <= bound[:m]), (k, out_dtype, m)
    big = layer(x33)                                 # m = 33: the block kernel
    assert np.array_equal(_bits(big), _bits(packed.linear(x33, pt, bias=bd, out_dtype=out_dtype, kernel="block")))
    assert np.all(np.abs(big.float().cpu().numpy().astype(np.float64) - want) <= bound), (k, out_dtype)


# ----------------------------------------------------------------------------- blobs that are not there

def _guard_case():
    m, n, k = 5, 70, 300
    pt, what, b = _grid_weight(n, k, "random")
    x = np.random.default_rng(1000 * m + 10 * n + k).integers(-4, 5, size=(m, k)).astype(np.float32)
    _grid_preconditions(x, what, b.astype(np.float64))
    return m, n, k, pt, what, b, x


def _zeroed(what, tiles_w, tiles):
    out = what.copy()
    for t in tiles:
        tr, tc = divmod(int(t), tiles_w)
        out[32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = 0.0
    return out


def _guarded_outputs_equal(x, pt, tables, n, b, what_left):
    """Both kernels (the skinny one at split 1 and at the library's split) through `tables`, with and without bias, against the float64
    product with `what_left`.  pt.data is the whole stream: a kernel without the guard reads real bytes and the comparison fails."""
    m, k = x.shape
    assert pt.data.numel() == pt.nbytes == pt.tables().nbytes                # never a shorter buffer
    b64 = b.astype(np.float64)
    nob_want = x.astype(np.float64) @ what_left.T
    assert np.array_equal(nob_want.astype(np.float32).astype(np.float64), nob_want)
    bd = torch.from_numpy(b.copy()).cuda()
    xd = _x_dev(x)
    lib = _library_split(m, n, k)
    assert lib > 1
    for bias, want in ((bd, nob_want + b64[None, :]), (None, nob_want)):
        got = {"block": hb.packed_linear(xd, pt.data, tables, n, bias=bias)}
        for split in (1, lib, 0):
            got[f"skinny, split {split}"] = hb.packed_linear_skinny(xd, pt.data, tables, n, bias=bias, split=split)
        for name, y in got.items():
            g = y.cpu().numpy().astype(np.float64)
            assert np.array_equal(g, want), (name, bias is not None, np.argwhere(g != want)[:4])


def test_a_blob_past_packed_bytes_reads_as_zeros():
    m, n, k, pt, what, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    tiles = tiles_h * tiles_w
    t_star = tiles - 3                               # (2, 7): of the first ring round of its run; (2, 8) and (2, 9) are of the second
    assert divmod(t_star, tiles_w) == (tiles_h - 1, 7)
    cut = int(pt.offsets[t_star + 1]) * 64 - 64      # 64 bytes short of the end of tile t*: it and every later tile do not fit
    assert cut >= tiles * TILE_BYTES[3]              # the entries refuse less
    assert int(pt.offsets[t_star]) * 64 + TILE_BYTES[int(pt.map.reshape(-1)[t_star])] == cut + 64 and cut < pt.nbytes
    short = copy.copy(pt.tables())                   # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    gone = range(t_star, tiles)
    what_left = _zeroed(what, tiles_w, gone)
    assert np.any(what[64:, 32 * 7:] != 0) and not np.any(what_left[64:, 32 * 7:])
    assert np.array_equal(what_left[:64], what[:64]) and np.array_equal(what_left[:, :32 * 7], what[:, :32 * 7])
    _guarded_outputs_equal(x, pt, short, n, b, what_left)
    assert pt.tables().nbytes == pt.nbytes                                                       # the shared tables were not touched


def test_a_tile_whose_map_code_is_no_format_reads_as_zeros():
    m, n, k, pt, what, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    tables = hb.PackedTables.on_device(pt.map, pt.offsets)                                       # a private copy: checked on the host first
    t_first, t_second = 0 * tiles_w + 3, 1 * tiles_w + 9                                         # ring rounds 1 and 2 of their runs at split 1
    assert t_first % tiles_w < 8 <= t_second % tiles_w
    tables.map_dev[t_first] = 4
    tables.map_dev[t_second] = -1
    assert tables.map_dev.cpu().numpy().tolist().count(4) == 1 and int(tables.map_dev[t_second]) == -1
    what_left = _zeroed(what, tiles_w, (t_first, t_second))
    assert np.count_nonzero(what_left != what) > 0 and np.count_nonzero(what_left != what) <= 2 * 32 * 32
    _guarded_outputs_equal(x, pt, tables, n, b, what_left)
    assert np.array_equal(pt.tables().map_dev.cpu().numpy(), pt.map.reshape(-1))                 # the shared tables were not touched
