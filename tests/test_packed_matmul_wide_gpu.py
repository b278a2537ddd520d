"""GPU: the wide-block product with a packed (k, n) matrix — packed_wide_kernel<.., WT = true> of csrc/mtq_packed.hip (wide_block with its W side
fed from the k × n stream) — and what packed.py builds on it: matmul_wide, and matmul(kernel="auto") / PackedMatmul(kernel="auto").

Names: W is the (n, k) weight as stored, P̂ its packed transpose (k, n), the map is over Wᵀ's grid ceil(k/32) × ceil(n/32).

The block is 128 (M) × 128 (N) × 64 (K); wave w stages tile column n0 / 32 + w, two tile rows a step.  The shapes are the smallest that
cross every boundary of it:

  m = 1, 33, 257, 300   a row block; a second 32-row MFMA block; a third row block of one row; ragged inside an MFMA block;
  n = 40                one column block, second tile column ragged, waves 2 and 3 without tiles;
  n = 200               a second column block, 7 tile columns, the last ragged, its fourth wave without a tile;
  k = 33                one step whose second tile row holds one k-row: the prologue's steps == 1 path;
  k = 100               two steps, last tile row ragged;
  k = 300               five steps, odd: both register sets and both images several times;
  k = 104, 320          a contiguous X with k % 8 == 0, the 16-byte X path; one n = 72 case among them;
  (300, 200, 2100)      33 steps, once.

Maps: random over all four codes, all-bfp4, all-bf16.

  * bit contract: matmul_wide == matmul(kernel="block") on the same PackedTensor, on the words (NaN-aware on the specials weight): both
    output types, with and without bias, X contiguous and at an odd pitch with an unaligned first element, y pitched with sentinels that
    stay, every call twice;
  * padding: the groups of k-rows at or past k of the last tile row overwritten with bytes that decode to NaN / Inf: the output still
    equals the block kernel's on the altered stream (and on the clean one) and has no NaN;
  * independent of the block kernel: the integer grid (tests/packed_cases.py, preconditions asserted on the CPU) EQUALS the float64
    product; one-hot rows X = 2ˢ·I at m = k = 300 return expected_bits(Wᵀ, map) at every (k, n); one flipped code byte changes exactly
    its output;
  * guards over buffers that stay whole: packed_bytes cut short of the last tile, map codes 4 and −1: that tile multiplies as zeros,
    every other output is the exact product;
  * routing: "auto" at m = 300 gives the block kernel's bits whatever the gate is; m = 0 is empty; n = 1 and k = 1 work.
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
SHAPES = [(m, n, k) for m in (1, 33, 257, 300) for n in (40, 200) for k in (33, 100, 300)] + [(300, 200, 2100)]
SHAPES += [(1, 200, 320), (33, 40, 104), (257, 72, 104), (300, 200, 320)]       # k % 8 == 0: the 16-byte loads of X
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def _maps(n, k):
    """Maps over Wᵀ's grid."""
    return (("random", random_map((k, n), n + k)), ("bfp4", uniform_map((k, n), 2)), ("bf16", uniform_map((k, n), 0)))


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _bits(t) -> np.ndarray:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(got, want, nan_aware, what):
    g, w = _bits(got), _bits(want)
    if nan_aware:
        gn, wn = torch.isnan(got).cpu().numpy(), torch.isnan(want).cpu().numpy()
        assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:4])
        g, w = np.where(gn, 0, g), np.where(wn, 0, w)
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:4])


def _phat(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """P̂ (k, n) as float64, from the oracle: the row-layout reconstruction of Wᵀ."""
    return expected_bits(np.ascontiguousarray(w.T), amap).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _weights(n, k, kind, which):
    """(P̂ on the device, bias) — made once, never written to."""
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", 7 * n + k, (n, k))
    amap = next(a for name, a in _maps(n, k) if name == which)
    return packed.pack_transposed(w, amap, backend="hip"), torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda()


@functools.lru_cache(maxsize=None)
def _x(m, k):
    x = _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 40))
    pitched = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    pitched[:, 1:1 + k] = x
    view = pitched[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and (m == 1 or view.stride(0) % 8 != 0)   # the scalar load path, whatever k is
    if k % 8 == 0:
        assert x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0                 # and the 16-byte one
    return x, view


def _into_sentinels(xd, pt, n, bias, dtype):
    """hb.packed_matmul_wide into a pitched view of a buffer of sentinels → the (m, n) result; the columns and rows around it stay."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_matmul_wide(xd, pt.data, pt.tables(), n, bias=bias, out_dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = buf.float().cpu().numpy()
    inside = np.zeros(whole.shape, dtype=bool)
    inside[1:1 + m, 2:2 + n] = True
    assert np.all(whole[~inside] == sentinel), (m, n, np.argwhere((whole != sentinel) & ~inside)[:4])
    return out


def _bit_contract(m, n, k, kind, names):
    plain, pitched = _x(m, k)
    for which in names:
        pt, bd = _weights(n, k, kind, which)
        for layout, xd in (("contiguous", plain), ("pitched", pitched)):
            for out_dtype, dtype in DTYPES:
                for bias in (None, bd):
                    what = (m, n, k, kind, which, layout, out_dtype, bias is not None)
                    want = packed.matmul(xd, pt, bias=bias, out_dtype=out_dtype, kernel="block")
                    got = packed.matmul_wide(xd, pt, bias=bias, out_dtype=out_dtype)
                    assert got.dtype == dtype and tuple(got.shape) == (m, n)
                    _same(got, want, kind == "specials", what)
                    _same(packed.matmul_wide(xd, pt, bias=bias, out_dtype=out_dtype), got, kind == "specials", what + ("again",))
                    _same(_into_sentinels(xd, pt, n, bias, dtype), want, kind == "specials", what + ("pitched y",))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_matmul_wide_is_the_block_kernel_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy", ("random", "bfp4", "bf16"))
    if k <= 320:
        _bit_contract(m, n, k, "specials", ("random",))


# ----------------------------------------------------------------------------- padding: k-rows at or past k are zeros in the image

def _poisoned(pt, k):
    """A copy of pt whose groups of the k-rows at or past k (the last tile row's padding) hold bytes that decode to NaN (bf16 tiles) or
    to Inf / NaN patterns (BFP tiles: exponent byte 255).  Every group is whole bytes of its blob in all four formats."""
    tiles_h, tiles_w = pt.map.shape
    rows = [r for r in range(32) if 32 * (tiles_h - 1) + r >= k]
    assert rows, "k must be ragged"
    data = pt.data.cpu().numpy().copy()
    for tc in range(tiles_w):
        f = int(pt.map[tiles_h - 1, tc])
        blob = int(pt.offsets[(tiles_h - 1) * tiles_w + tc]) * 64
        for r in rows:
            for g in (2 * r, 2 * r + 1):
                if f == 0:
                    data[blob + 32 * g: blob + 32 * g + 32] = np.tile(np.array([0xC0, 0x7F], dtype=np.uint8), 16)     # bf16 NaN 0x7FC0
                else:
                    per = (16, 8, 4)[f - 1]
                    data[blob + g] = 0xFF
                    data[blob + 64 + per * g: blob + 64 + per * (g + 1)] = 0x7F if f == 1 else 0x77 if f == 2 else 0x55
    bad = copy.copy(pt)
    bad.data = torch.from_numpy(data).cuda()
    # the altered bytes do decode to non-finite values, and only in the padding
    words = packed.decode(data, pt.map, pt.offsets, 32 * tiles_h, 32 * tiles_w).view(np.float32)
    clean = packed.decode(pt.data.cpu().numpy(), pt.map, pt.offsets, 32 * tiles_h, 32 * tiles_w).view(np.float32)
    assert not np.any(np.isfinite(words[k:, :])) and np.array_equal(words[:k].view(np.uint32), clean[:k].view(np.uint32))
    return bad


@pytest.mark.parametrize("m,n,k", [(33, 40, 33), (257, 200, 100), (300, 200, 300), (33, 72, 104)])
def test_k_rows_past_k_are_zeros_in_the_image_whatever_the_stream_holds(m, n, k):
    plain, pitched = _x(m, k)
    for which in ("bf16", "random"):
        pt, bd = _weights(n, k, "heavy", which)
        bad = _poisoned(pt, k)
        for xd in (plain, pitched):
            for out_dtype, _dtype in DTYPES:
                got = packed.matmul_wide(xd, bad, bias=bd, out_dtype=out_dtype)
                assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got.float()).all()), (m, n, k, which, out_dtype)
                _same(got, packed.matmul(xd, bad, bias=bd, out_dtype=out_dtype, kernel="block"), False, (m, n, k, which, "altered"))
                _same(got, packed.matmul_wide(xd, pt, bias=bd, out_dtype=out_dtype), False, (m, n, k, which, "clean"))


# ----------------------------------------------------------------------------- exact arithmetic, independent of the block kernel

@pytest.mark.parametrize("m", [1, 33, 257, 300])
def test_matmul_wide_integer_grid_is_exact(m):
    for n in (40, 200):
        for k in (33, 100, 300):
            x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
            for _name, amap in _maps(n, k):
                phat = _phat(w, amap)                                       # (k, n)
                _grid_preconditions(x, phat.T, b.astype(np.float64))
                want = x.astype(np.float64) @ phat + b.astype(np.float64)[None, :]
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
                pt = packed.pack_transposed(w, amap, backend="hip")
                bd = torch.from_numpy(b).cuda()
                got = packed.matmul_wide(_x_dev(x), pt, bias=bd).cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, _name, np.argwhere(got != want)[:4])
                nob = packed.matmul_wide(_x_dev(x), pt).cpu().numpy()
                assert np.array_equal(nob.astype(np.float64), want - b.astype(np.float64)[None, :]), (m, n, k, _name)
                yb = packed.matmul_wide(_x_dev(x), pt, bias=bd, out_dtype="bfloat16")
                assert np.array_equal(yb.float().cpu().numpy(), torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16).float().numpy())


def _one_hot_mismatches(n, k, s, seed, corrupt=False):
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((k, n), seed + 1).copy()
    amap[0, 0] = 1
    pt = packed.pack_transposed(w, amap, backend="hip")
    if corrupt:     # one code byte of tile 0 (bfp8): element (row 0, column 5) of P̂ changes its last mantissa bit
        pt.data[int(pt.offsets[0]) * 64 + 64 + 5] ^= 0x01
    x = (np.eye(k, dtype=np.float32) * np.float32(2.0 ** s))
    y = packed.matmul_wide(_x_dev(x), pt).cpu().numpy().astype(np.float64)
    want = (2.0 ** s) * _phat(w, amap)
    assert y.shape == want.shape == (k, n)
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return np.argwhere(y != want)


@pytest.mark.parametrize("n,s", [(200, 3), (40, -2)])
def test_matmul_wide_one_hot_pins_every_position(n, s):
    bad = _one_hot_mismatches(n, 300, s, 50 + n)
    assert bad.size == 0, bad[:8]


def test_matmul_wide_one_flipped_code_byte_changes_exactly_its_output():
    bad = _one_hot_mismatches(200, 300, 3, 120, corrupt=True)
    assert [tuple(r) for r in bad] == [(0, 5)]          # Y[k = 0, n = 5] alone


# ----------------------------------------------------------------------------- guards and boundaries

@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 257, 200, 100                              # P̂'s grid 4 × 7
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
    """mtq_packed_matmul_wide through `tables`, with and without bias, against the exact product with `phat_left`.  pt.data is the whole
    stream: a kernel without the guard reads real bytes and the comparison fails."""
    assert pt.data.numel() == pt.nbytes == pt.tables().nbytes                # never a shorter buffer
    b64 = b.astype(np.float64)
    nob_want = x.astype(np.float64) @ phat_left
    assert np.array_equal(nob_want.astype(np.float32).astype(np.float64), nob_want)
    bd = torch.from_numpy(b.copy()).cuda()
    got = hb.packed_matmul_wide(_x_dev(x), pt.data, tables, n, bias=bd).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, nob_want + b64[None, :]), np.argwhere(got != nob_want + b64[None, :])[:4]
    nob = hb.packed_matmul_wide(_x_dev(x), pt.data, tables, n).cpu().numpy().astype(np.float64)
    assert np.array_equal(nob, nob_want), np.argwhere(nob != nob_want)[:4]


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
    t_a, t_b = 0 * tiles_w + 3, 3 * tiles_w + 4                              # K steps 0 and 1, column blocks 0 (wave 3) and 1 (wave 0)
    tables.map_dev[t_a] = 4
    tables.map_dev[t_b] = -1
    left = _zeroed(phat, tiles_w, (t_a, t_b))
    assert 0 < np.count_nonzero(left != phat) <= 2 * 32 * 32
    _guarded_outputs_equal(x, pt, tables, n, b, left)
    assert np.array_equal(pt.tables().map_dev.cpu().numpy(), pt.map.reshape(-1))                 # the shared tables were not touched


def test_auto_gives_the_block_kernels_bits_whatever_the_gate_is(monkeypatch):
    m, n, k = 300, 200, 300
    xd, _view = _x(m, k)
    pt, bd = _weights(n, k, "heavy", "random")
    assert hb.has_packed_matmul_wide()
    for out_dtype, _dtype in DTYPES:
        want = packed.matmul(xd, pt, bias=bd, out_dtype=out_dtype, kernel="block")
        for gate in (packed.AUTO_MATMUL_WIDE_MIN_M, None, 64, m, m + 1):
            monkeypatch.setattr(packed, "AUTO_MATMUL_WIDE_MIN_M", gate)
            _same(packed.matmul(xd, pt, bias=bd, out_dtype=out_dtype, kernel="auto"), want, False, ("auto", gate, out_dtype))
            mod = packed.PackedMatmul(pt, bias=bd, out_dtype=out_dtype, kernel="auto")
            _same(mod(xd.reshape(2, m // 2, k)).reshape(m, n), want, False, ("module", gate, out_dtype))


def test_boundaries():
    pt, _bd = _weights(72, 104, "heavy", "random")
    for out_dtype, dtype in DTYPES:
        empty = packed.matmul_wide(torch.zeros((0, 104), dtype=torch.bfloat16, device="cuda"), pt, out_dtype=out_dtype)
        assert tuple(empty.shape) == (0, 72) and empty.dtype == dtype
    for n, k in ((1, 100), (72, 1), (1, 1)):             # one column, one k-row
        xg, wg, bg = _grid_case(33, n, k, 77 + n + k)
        a = random_map((k, n), n + k)
        phat = _phat(wg, a)
        _grid_preconditions(xg, phat.T, bg.astype(np.float64))
        got = packed.matmul_wide(_x_dev(xg), packed.pack_transposed(wg, a, backend="hip"), bias=torch.from_numpy(bg).cuda()).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), xg.astype(np.float64) @ phat + bg.astype(np.float64)[None, :]), (n, k)
    x6 = torch.zeros((6, 104), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.packed_matmul_wide(x6, pt.data, pt.tables(), 20)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_matmul_wide(x6.float(), pt.data, pt.tables(), 72)
