"""GPU: the skinny (split-K, m <= 32) product with a packed (k, n) matrix — packed_matmul_skinny_kernel of csrc/mtq_packed.hip — and
what packed.py builds on it.

Names: W is the (n, k) weight as stored, P̂ its packed transpose (k, n), the map is over Wᵀ's grid tiles_kh × tiles_nw =
ceil(k/32) × ceil(n/32).  A wave takes one (K slice, tile column) unit, four waves to a workgroup, a ring of 8 tiles in flight, the map
codes and offsets of 64 tiles per load.  The shapes are the smallest that cross every boundary of that:

  m = 1, 5, 32      one row, a row in the upper lane half's outputs, all rows;
  n = 40            a ragged second tile column;
  n = 72            three units in a four-wave workgroup: one wave exits;
  n = 200           a second workgroup of three units;
  k = 100           the element-wise X path, a ragged last tile row;
  k = 104           the 16-byte X path, ragged;
  k = 288, 300      a second ring round of one tile and of two; the library's split is 2;
  k = 2100          a second 64-tile chunk; the library's split is 16;
  (72, 4200)        slices that start off zero and cross a chunk, the library's split is 33, once;
  (19200, 512)      the kSkinnyUnits side of the split rule (600 tile columns: split 3), once.

Maps: random over all four codes, all-bfp4, all-bfp2, all-bf16.  Splits: 0 (the library's), 1, 2, 5, tiles_kh, tiles_kh + 3.

  * bit contract: matmul(kernel="skinny", split=s) == linear(kernel="skinny", split=s) on the all-bf16 row-layout packing of
    unpack(P̂)ᵀ, on the words (NaN-aware on the specials weight): both output types, with and without bias, X contiguous and at an odd
    pitch, y pitched with sentinels, twice on a workspace pre-filled with NaN patterns;
  * exact arithmetic, independent of any other kernel: the integer grid (tests/packed_cases.py, preconditions asserted on the CPU)
    EQUALS the float64 product at every split; one-hot rows of X return P̂ for every (k, n) position at k = 300 and 2100; one flipped
    code byte changes exactly its output, in a tile of the second ring round and in a tile of the second chunk;
  * accuracy on heavy-tailed data: |Y − Y₆₄| ≤ (k + 2)·2⁻²⁴·(Σ|x||ŵ| + |b|) at k up to 4200;
  * guards over buffers that stay whole: packed_bytes cut short of a tile, map codes 4 and −1: that tile multiplies as zeros and every
    other output is the exact product; the bytes of the padding k-rows (k = 100: rows 100..127) overwritten: Y keeps its bits;
  * PackedMatmul(kernel="skinny") on its kept workspace equals matmul(kernel="skinny"); kernel="auto" follows
    AUTO_MATMUL_SKINNY_MAX_M; m = 0 is empty, n = 1 and k = 1 work.
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
from tests.packed_cases import TILE_BYTES, _grid_case, _grid_preconditions, expected_bits, random_map, specials, uniform_map

pytestmark = pytest.mark.gpu
MS, NS, KS = (1, 5, 32), (40, 72, 200), (100, 104, 288, 300, 2100)
NK = [(n, k) for n in NS for k in KS] + [(72, 4200)]
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
MAPS = ("random", "bfp4", "bfp2", "bf16")


def _splits(k):
    tiles_kh = -(-k // 32)
    return (0, 1, 2, 5, tiles_kh, tiles_kh + 3)


def _map(n, k, which):
    """A map over Wᵀ's grid."""
    return random_map((k, n), n + k) if which == "random" else uniform_map((k, n), {"bf16": 0, "bfp4": 2, "bfp2": 3}[which])


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want, nan_aware, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = _bits(got), _bits(want)
    if nan_aware:
        gn, wn = torch.isnan(got), torch.isnan(want)
        assert torch.equal(gn, wn), (what, "NaN positions", torch.nonzero(gn != wn)[:4].tolist())
        g, w = torch.where(gn, 0, g), torch.where(wn, 0, w)
    assert torch.equal(g, w), (what, torch.nonzero(g != w)[:4].tolist())


def _phat(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """P̂ (k, n) as float64, from the oracle: the row-layout reconstruction of Wᵀ."""
    return expected_bits(np.ascontiguousarray(w.T), amap).view(np.float32).astype(np.float64)


def _nan_workspace(m, n, k, split):
    """A workspace of the size the call needs (at least 16 bytes), every word a NaN pattern."""
    need = hb.packed_matmul_skinny_workspace_bytes(m, n, k, split)
    assert need == hb.packed_linear_skinny_workspace_bytes(m, n, k, split)
    return torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device="cuda")


def test_the_library_split_of_the_shapes_is_what_the_docstring_says():
    f = hb.packed_matmul_skinny_workspace_bytes
    for n, k, split in ((72, 100, 1), (72, 104, 1), (72, 288, 2), (72, 300, 2), (200, 2100, 16), (72, 4200, 33), (19200, 512, 3)):
        assert f(5, n, k, 0) == f(5, n, k, split) and (split == 1 or f(5, n, k, 0) != f(5, n, k, split - 1)), (n, k, split)


# ----------------------------------------------------------------------------- the bit contract

@functools.lru_cache(maxsize=None)
def _weights(n, k, kind, which):
    """(P̂ on the device, the all-bf16 row-layout packing of unpack(P̂)ᵀ, bias) — made once, never written to.  The unpacked matrix comes
    from the NumPy decoder on the device's bytes."""
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", 7 * n + k, (n, k))
    amap = _map(n, k, which)
    pt = packed.pack_transposed(w, amap, backend="hip")
    host = packed.decode(pt.data.cpu().numpy(), pt.map, pt.offsets, k, n)                                  # (k, n) words
    assert np.array_equal(host, expected_bits(np.ascontiguousarray(w.T), amap)) and np.all(host & np.uint32(0xFFFF) == 0)
    ref = packed.pack(np.ascontiguousarray(host.T).view(np.float32), uniform_map((n, k), 0), backend="hip")
    assert np.array_equal(packed.decode(ref.data.cpu().numpy(), ref.map, ref.offsets, n, k), host.T)       # lossless
    return pt, ref, torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda()


@functools.lru_cache(maxsize=None)
def _x(m, k):
    x = _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 40))
    pitched = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    pitched[:, 1:1 + k] = x
    view = pitched[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and (m == 1 or view.stride(0) % 8 != 0)   # the scalar load path
    return x, view


def _into_sentinels(xd, pt, n, bias, dtype, split, ws):
    """hb.packed_matmul_skinny into a pitched view of a buffer of sentinels → the (m, n) result; what lies around it stays."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_matmul_skinny(xd, pt.data, pt.tables(), n, bias=bias, out_dtype=dtype, out=out, split=split, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    inside = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    inside[1:1 + m, 2:2 + n] = True
    assert bool(torch.all(buf[~inside] == sentinel)), (m, n, split)
    return out


def _bit_contract(m, n, k, kind, names, splits=None):
    plain, pitched = _x(m, k)
    for which in names:
        pt, ref, bd = _weights(n, k, kind, which)
        for split in (_splits(k) if splits is None else splits):
            ws = _nan_workspace(m, n, k, split)
            for layout, xd in (("contiguous", plain), ("pitched", pitched)):
                for out_dtype, dtype in DTYPES:
                    for bias in (None, bd):
                        what = (m, n, k, kind, which, split, layout, out_dtype, bias is not None)
                        want = packed.linear(xd, ref, bias=bias, out_dtype=out_dtype, kernel="skinny", split=split)
                        got = packed.matmul(xd, pt, bias=bias, out_dtype=out_dtype, kernel="skinny", split=split, workspace=ws)
                        assert got.dtype == dtype and tuple(got.shape) == (m, n)
                        _same(got, want, kind == "specials", what)
                        again = packed.matmul(xd, pt, bias=bias, out_dtype=out_dtype, kernel="skinny", split=split, workspace=ws)
                        _same(again, got, kind == "specials", what + ("again",))
                        _same(_into_sentinels(xd, pt, n, bias, dtype, split, ws), want, kind == "specials", what + ("pitched y",))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n,k", NK)
def test_skinny_matmul_is_the_skinny_linear_on_the_transposed_weight_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy", MAPS)
    if k <= 300:
        _bit_contract(m, n, k, "specials", ("random",))


def test_the_units_side_of_the_split_rule_bit_for_bit():
    """n = 19200, k = 512: 600 tile columns, so the library's split is 2048 // 600 = 3, not 16 // 4.  The pair is made on the device
    (unpack, tested elsewhere), and the grid's product is exact in float64."""
    m, n, k = 5, 19200, 512
    x, w, b = _grid_case(m, n, k, 99)
    amap = random_map((k, n), 98)
    pt = packed.pack_transposed(torch.from_numpy(w).cuda(), amap, backend="hip")
    phat = packed.unpack(pt, backend="hip", dtype="bfloat16")                    # (k, n)
    ref = packed.pack(phat.t().contiguous(), uniform_map((n, k), 0), backend="hip")
    xd, bd = _x_dev(x), torch.from_numpy(b).cuda()
    p64 = phat.double()
    assert float(p64.abs().max()) <= 1.0 and bool(torch.all(p64 * 256 == torch.round(p64 * 256)))   # the grid's preconditions, on P̂
    want64 = xd.double() @ p64 + bd.double()[None, :]
    for split in (0, 3, 1, 16):
        ws = _nan_workspace(m, n, k, split)
        for out_dtype, _dtype in DTYPES:
            got = packed.matmul(xd, pt, bias=bd, out_dtype=out_dtype, kernel="skinny", split=split, workspace=ws)
            _same(got, packed.linear(xd, ref, bias=bd, out_dtype=out_dtype, kernel="skinny", split=split), False, (split, out_dtype))
            if out_dtype == "float32":
                assert torch.equal(got.double(), want64), split
    assert hb.packed_matmul_skinny_workspace_bytes(m, n, k, 0) == hb.packed_matmul_skinny_workspace_bytes(m, n, k, 3)


# ----------------------------------------------------------------------------- exact, independent of any other kernel

@pytest.mark.parametrize("n,k", NK)
def test_skinny_matmul_integer_grid_is_exact_at_every_split(n, k):
    for m in MS:
        x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
        xd, bd = _x_dev(x), torch.from_numpy(b).cuda()
        for which in MAPS:
            amap = _map(n, k, which)
            phat = _phat(w, amap)                                           # (k, n)
            _grid_preconditions(x, phat.T, b.astype(np.float64))
            want = x.astype(np.float64) @ phat + b.astype(np.float64)[None, :]
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
            wantb = torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16).float().numpy()
            pt = packed.pack_transposed(w, amap, backend="hip")
            for split in _splits(k):
                ws = _nan_workspace(m, n, k, split)
                got = packed.matmul(xd, pt, bias=bd, kernel="skinny", split=split, workspace=ws).cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, which, split, np.argwhere(got != want)[:4])
                nob = packed.matmul(xd, pt, kernel="skinny", split=split, workspace=ws).cpu().numpy()
                assert np.array_equal(nob.astype(np.float64), want - b.astype(np.float64)[None, :]), (m, n, k, which, split)
                yb = packed.matmul(xd, pt, bias=bd, out_dtype="bfloat16", kernel="skinny", split=split, workspace=ws)
                assert np.array_equal(yb.float().cpu().numpy(), wantb), (m, n, k, which, split)


def _one_hot(pt, k, n, s, split):
    """Y for X = 2^s · I, 32 rows of the identity to a call: (k, n) float64."""
    eye = torch.eye(k, dtype=torch.bfloat16, device="cuda") * (2.0 ** s)
    ws = _nan_workspace(32, n, k, split)
    rows = [packed.matmul(eye[r: r + 32], pt, kernel="skinny", split=split, workspace=ws) for r in range(0, k, 32)]
    return torch.cat(rows).cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _one_hot_case(n, k, seed):
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((k, n), seed + 1).copy()
    amap[8, 1] = amap[-2, min(2, amap.shape[1] - 1)] = 1  # bfp8 where the flipped bytes go (n = 200: tile columns 1 and 2)
    return w, amap, _phat(w, amap)


@pytest.mark.parametrize("n,k,s", [(72, 300, 3), (200, 300, -2), (200, 2100, 0), (40, 2100, 1)])
def test_skinny_matmul_one_hot_pins_every_position(n, k, s):
    w, amap, phat = _one_hot_case(n, k, 50 + n)
    pt = packed.pack_transposed(w, amap, backend="hip")
    want = (2.0 ** s) * phat
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    for split in (0, 1, 5):
        y = _one_hot(pt, k, n, s, split)
        assert y.shape == want.shape == (k, n)
        assert np.array_equal(y, want), (split, np.argwhere(y != want)[:8])


@pytest.mark.parametrize("k,tr", [(300, 8), (2100, 64)])
def test_one_flipped_code_byte_changes_exactly_its_output(k, tr):
    """tr = 8: with split 1 the tile is the first of the unit's second ring round; tr = 64 (= tiles_kh - 2): the first of its second
    64-tile chunk.  One code byte of the bfp8 tile (tr, tc): element (row 3, column 21) of the tile changes its last mantissa bit."""
    n, tc = 200, 1 if tr == 8 else 2
    w, amap, phat = _one_hot_case(n, k, 50 + n)
    assert amap[tr, tc] == 1 and (tr == 8 or tr == amap.shape[0] - 2)
    pt = packed.pack_transposed(w, amap, backend="hip")
    t = tr * amap.shape[1] + tc
    pt.data[int(pt.offsets[t]) * 64 + 64 + 32 * 3 + 21] ^= 0x01
    for split in (1, 0):
        bad = np.argwhere(_one_hot(pt, k, n, 0, split) != phat)
        assert [tuple(r) for r in bad] == [(32 * tr + 3, 32 * tc + 21)], (split, bad[:8])


@pytest.mark.parametrize("m,n,k", [(1, 72, 300), (5, 200, 2100), (32, 40, 2100), (32, 72, 4200)])
def test_skinny_matmul_random_is_within_the_f32_accumulation_bound(m, n, k):
    w = gen("heavy_f32", 60 + m, (n, k))
    x = to_bf16_valued(gen("normal_f32", 61 + m, (m, k)) * 40)
    b = gen("normal_f32", 62 + m, (n,))
    amap = random_map((k, n), 63 + m)
    phat = _phat(w, amap)
    want = x.astype(np.float64) @ phat + b.astype(np.float64)[None, :]
    bound = (k + 2) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(phat) + np.abs(b).astype(np.float64)[None, :])
    pt = packed.pack_transposed(w, amap, backend="hip")
    bd = torch.from_numpy(b).cuda()
    wide = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    wide[:, 1:1 + k] = _x_dev(x)
    for split in (0, 1, 5):
        for xd in (_x_dev(x), wide[:, 1:1 + k]):
            got = packed.matmul(xd, pt, bias=bd, kernel="skinny", split=split).cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            print(f"m={m} n={n} k={k} split={split}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound), (m, n, k, split, float(np.max(err / np.maximum(bound, 1e-300))))
            yb = packed.matmul(xd, pt, bias=bd, out_dtype="bfloat16", kernel="skinny", split=split)
            errb = np.abs(yb.float().cpu().numpy().astype(np.float64) - want)
            assert np.all(errb <= bound * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want)), (m, n, k, split)


# ----------------------------------------------------------------------------- guards and boundaries

@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 32, 200, 100                                # P̂'s grid 4 × 7
    x, w, b = _grid_case(m, n, k, 4242)
    amap = random_map((k, n), 17).copy()
    amap[-1, -1] = 0                                     # the last tile is the largest blob: cutting it short cuts nothing else
    phat = _phat(w, amap)
    _grid_preconditions(x, phat.T, b.astype(np.float64))
    return m, n, k, packed.pack_transposed(w, amap, backend="hip"), phat, b, x


def _zeroed(phat, tiles_w, gone):
    left = phat.copy()
    for t in gone:
        tr, tc = divmod(int(t), tiles_w)
        left[32 * tr: 32 * tr + 32, 32 * tc: 32 * tc + 32] = 0.0
    return left


def _guarded_outputs_equal(x, pt, tables, n, b, phat_left):
    """mtq_packed_matmul_skinny through `tables` at every split, with and without bias, against the exact product with `phat_left`.
    pt.data is the whole stream: a kernel without the guard reads real bytes and the comparison fails."""
    assert pt.data.numel() == pt.nbytes == pt.tables().nbytes                # never a shorter buffer
    b64 = b.astype(np.float64)
    nob_want = x.astype(np.float64) @ phat_left
    assert np.array_equal(nob_want.astype(np.float32).astype(np.float64), nob_want)
    bd = torch.from_numpy(b.copy()).cuda()
    for split in _splits(x.shape[1]):
        got = hb.packed_matmul_skinny(_x_dev(x), pt.data, tables, n, bias=bd, split=split).cpu().numpy().astype(np.float64)
        assert np.array_equal(got, nob_want + b64[None, :]), (split, np.argwhere(got != nob_want + b64[None, :])[:4])
        nob = hb.packed_matmul_skinny(_x_dev(x), pt.data, tables, n, split=split).cpu().numpy().astype(np.float64)
        assert np.array_equal(nob, nob_want), (split, np.argwhere(nob != nob_want)[:4])


def test_a_blob_past_packed_bytes_multiplies_as_zeros():
    m, n, k, pt, phat, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    tiles = tiles_h * tiles_w
    cut = pt.nbytes - 64                                 # 64 bytes short of the end of the last tile
    assert cut >= tiles * TILE_BYTES[3] and int(pt.offsets[tiles - 1]) * 64 < cut
    short = copy.copy(pt.tables())                       # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    left = _zeroed(phat, tiles_w, (tiles - 1,))
    assert np.any(left != phat) and np.array_equal(left[:96], phat[:96]) and np.array_equal(left[:, :192], phat[:, :192])
    _guarded_outputs_equal(x, pt, short, n, b, left)
    assert pt.tables().nbytes == pt.nbytes                                   # the shared tables were not touched


def test_a_tile_whose_map_code_is_no_format_multiplies_as_zeros():
    m, n, k, pt, phat, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    tables = hb.PackedTables.on_device(pt.map, pt.offsets)                   # a private copy: checked on the host first
    t_a, t_b = 0 * tiles_w + 3, 2 * tiles_w + 4                              # tile rows 0 and 2, the fourth and the fifth unit of a slice
    tables.map_dev[t_a] = 4
    tables.map_dev[t_b] = -1
    left = _zeroed(phat, tiles_w, (t_a, t_b))
    assert 0 < np.count_nonzero(left != phat) <= 2 * 32 * 32
    _guarded_outputs_equal(x, pt, tables, n, b, left)
    assert np.array_equal(pt.tables().map_dev.cpu().numpy(), pt.map.reshape(-1))                 # the shared tables were not touched


def test_the_bytes_of_padding_k_rows_mean_nothing():
    """k = 100: rows 100..127 of the last tile row are padding.  Their code bytes (and, stronger, their exponent bytes) are overwritten
    with 0xFF - NaNs in a bf16 tile, the largest codes under the largest exponent in a BFP tile: Y keeps every bit."""
    m, n, k, pt, phat, b, x = _guard_case()
    tiles_h, tiles_w = pt.map.shape
    data = pt.data.clone()
    for tc in range(tiles_w):
        t = (tiles_h - 1) * tiles_w + tc
        f, base = int(pt.map[tiles_h - 1, tc]), int(pt.offsets[t]) * 64
        g0 = 2 * (k - 32 * (tiles_h - 1))                                    # the first padding group: row 4 of the tile
        if f == 0:
            data[base + 32 * g0: base + 2048] = 0xFF
        else:
            per = {1: 16, 2: 8, 3: 4}[f]
            data[base + g0: base + 64] = 0xFF
            data[base + 64 + per * g0: base + TILE_BYTES[f]] = 0xFF
    assert int((data != pt.data).sum()) > tiles_w * 28 * 8
    nan_rows = packed.unpack(packed.PackedTensor((128, n), ("nd", (128, n)), 128, n, pt.map, pt.offsets, data, _tables=pt.tables()), backend="hip")
    assert bool(torch.isnan(nan_rows[100:]).any()) and np.array_equal(nan_rows[:100].cpu().numpy().astype(np.float64), phat)   # the bytes took
    xd, bd = _x_dev(x), torch.from_numpy(b).cuda()
    want = x.astype(np.float64) @ phat + b.astype(np.float64)[None, :]
    for split in _splits(k):
        for out_dtype, _dtype in DTYPES:
            clean = hb.packed_matmul_skinny(xd, pt.data, pt.tables(), n, bias=bd, out_dtype=_dtype, split=split)
            dirty = hb.packed_matmul_skinny(xd, data, pt.tables(), n, bias=bd, out_dtype=_dtype, split=split)
            _same(dirty, clean, False, (split, out_dtype))
            if out_dtype == "float32":
                assert np.array_equal(dirty.cpu().numpy().astype(np.float64), want), split


def test_the_module_keeps_one_workspace_and_auto_follows_the_constant():
    n, k = 72, 300
    pt, ref, bd = _weights(n, k, "heavy", "random")
    mod = packed.PackedMatmul(pt, bias=bd, out_dtype="bfloat16", kernel="skinny")
    assert mod.backend == "hip" and mod.kernel == "skinny" and (mod.in_features, mod.out_features) == (k, n)
    ws = mod._workspace
    assert ws is not None and ws.numel() == hb.packed_matmul_skinny_workspace_bytes(32, n, k) and ws.data_ptr() % 16 == 0
    ws.fill_(0xFF)                                       # its contents never need initialising
    for m in (1, 32, 5, 1):
        xd = _x(m, k)[0]
        want = packed.matmul(xd, pt, bias=bd, out_dtype="bfloat16", kernel="skinny")
        _same(mod(xd), want, False, m)
        _same(want, packed.linear(xd, ref, bias=bd, out_dtype="bfloat16", kernel="skinny"), False, (m, "the contract pair"))
        assert mod._workspace is ws
    y = mod(_x(32, k)[0].reshape(4, 8, k))
    assert tuple(y.shape) == (4, 8, n)
    _same(y.reshape(32, n), packed.matmul(_x(32, k)[0], pt, bias=bd, out_dtype="bfloat16", kernel="skinny"), False, "lead")
    with pytest.raises(hb.MtqError, match='kernel="skinny" takes m <= 32'):
        mod(torch.zeros((33, k), dtype=torch.bfloat16, device="cuda"))
    assert packed.PackedMatmul(pt)._workspace is None and packed.PackedMatmul(pt).kernel == "block"
    auto = packed.AUTO_MATMUL_SKINNY_MAX_M
    amod = packed.PackedMatmul(pt, bias=bd, kernel="auto")
    for m in (1, 5, 32, 33):
        xd = _x_dev(to_bf16_valued(gen("normal_f32", 5 + m, (m, k)) * 40))
        skinny = auto is not None and m <= auto
        want = packed.matmul(xd, pt, bias=bd, kernel="skinny" if skinny else "block")
        _same(packed.matmul(xd, pt, bias=bd, kernel="auto"), want, False, ("auto", m))
        _same(amod(xd), want, False, ("auto module", m))
    _same(packed.matmul(_x(5, k)[0], pt, bias=bd), packed.matmul(_x(5, k)[0], pt, bias=bd, kernel="block"), False, "the default is block")


def test_boundaries():
    n, k = 72, 100
    pt, _ref, _bd = _weights(n, k, "heavy", "random")
    for out_dtype, dtype in DTYPES:
        empty = packed.matmul(torch.zeros((0, k), dtype=torch.bfloat16, device="cuda"), pt, out_dtype=out_dtype, kernel="skinny")
        assert tuple(empty.shape) == (0, n) and empty.dtype == dtype
    assert tuple(packed.PackedMatmul(pt, kernel="skinny")(torch.zeros((0, k), dtype=torch.bfloat16, device="cuda")).shape) == (0, n)
    for n1, k1 in ((1, 100), (72, 1), (1, 1)):           # one column, one k-row
        xg, wg, bg = _grid_case(32, n1, k1, 77 + n1 + k1)
        a = random_map((k1, n1), n1 + k1)
        phat = _phat(wg, a)
        _grid_preconditions(xg, phat.T, bg.astype(np.float64))
        p1 = packed.pack_transposed(wg, a, backend="hip")
        for split in (0, 1, 3):
            got = packed.matmul(_x_dev(xg), p1, bias=torch.from_numpy(bg).cuda(), kernel="skinny", split=split).cpu().numpy()
            assert np.array_equal(got.astype(np.float64), xg.astype(np.float64) @ phat + bg.astype(np.float64)[None, :]), (n1, k1, split)
    xd = _x(5, k)[0]
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.packed_matmul_skinny(xd, pt.data, pt.tables(), 20)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_matmul_skinny(xd.float(), pt.data, pt.tables(), n)
    with pytest.raises(hb.MtqError, match="m <= 32"):
        hb.packed_matmul_skinny(torch.zeros((33, k), dtype=torch.bfloat16, device="cuda"), pt.data, pt.tables(), n)
    with pytest.raises(hb.MtqError, match="workspace"):
        hb.packed_matmul_skinny(xd, pt.data, pt.tables(), n, split=2, workspace=torch.zeros((16,), dtype=torch.uint8, device="cuda"))
