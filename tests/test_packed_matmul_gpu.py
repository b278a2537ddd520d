"""GPU: the packed transpose and the (k, n) product — pack_tiles_transposed_kernel, unpack_tiles_transposed_kernel and
packed_matmul_kernel of csrc/mtq_packed.hip — and what packed.py builds on them.

Names: W is the (n, k) weight as stored, P̂ its packed transpose (k, n), the map is over Wᵀ's grid ceil(k/32) × ceil(n/32).

The matmul block is 128 (M) × 64 (N) × 64 (K) over 32 × 32 tiles of 16-groups that run along n.  The shapes are the smallest that cross
every boundary of it:

  m = 1, 33, 130    one row, a second 32-row MFMA block of one row, a second workgroup row of two rows;
  n = 40            one column block whose second 32-column slot is ragged (8 of 32) and whose second tile column ends there;
  n = 72            a second column block with 8 columns: its second tile column and slot 1 are absent (zeros in the image);
  n = 200           four column blocks, the last ragged with an absent tile column;
  k = 100, 300      the element-wise X path, two and five K steps, the last tile row ragged (k-rows past k are zeros in the image);
  k = 104, 320      a contiguous X with k % 8 == 0: the 16-byte X path, ragged and whole;
  (130, 72, 2100)   33 steps, once.

Maps: random over all four codes (neighbouring lanes decode different formats), all-bfp4, all-bf16.

  * pack: the device stream == the emulation's bytes (pack of a contiguous Wᵀ) == mtq_pack_tiles on a contiguous device Wᵀ; float32 and
    bf16 storage, a pitched view, the specials tensor, every byte written;
  * unpack: float32 words == K3T's on the same W and map == expected_bits(Wᵀ, map)ᵀ; bf16 the upper halves; a pitched y keeps its
    sentinels;
  * bit contract: matmul == linear(kernel="block") on the all-bf16 row-layout packing of unpack(P̂)ᵀ, on the words (NaN-aware on the
    specials weight): both output types, with and without bias, X contiguous and at an odd pitch, y pitched with sentinels, twice;
  * exact arithmetic, independent of the block kernel: the integer grid (tests/packed_cases.py, preconditions asserted on the CPU)
    EQUALS the float64 product; one-hot rows of X return P̂ row by row, which pins the decode and the image position of every (k, n)
    element, and one flipped code byte of the stream changes exactly the output it should;
  * accuracy on heavy-tailed data: |Y − Y₆₄| ≤ (k + 2)·2⁻²⁴·(Σ|x||ŵ| + |b|);
  * guards over buffers that stay whole: packed_bytes cut short of the last tile, map codes 4 and −1: that tile multiplies as zeros,
    every other output is the exact product;
  * m = 0 is empty, n = 1 and k = 1 work, PackedMatmul equals matmul.
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
SHAPES = [(m, n, k) for m in (1, 33, 130) for n in (40, 72, 200) for k in (100, 300)] + [(130, 72, 2100)]
SHAPES += [(1, 72, 320), (33, 200, 104), (130, 40, 104), (130, 200, 320)]       # k % 8 == 0: the 16-byte loads of X
NK = [(40, 100), (72, 300), (200, 100), (1, 17), (70, 50)]                       # (n, k) of the pack / unpack tests
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def _maps(n, k):
    """Maps over Wᵀ's grid."""
    return (("random", random_map((k, n), n + k)), ("bfp4", uniform_map((k, n), 2)), ("bf16", uniform_map((k, n), 0)))


def _dev(x: np.ndarray, storage: str):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    if storage == "f32":
        return torch.from_numpy(u.view(np.float32).copy()).cuda()
    assert np.all(u & np.uint32(0xFFFF) == 0)
    return torch.from_numpy((u >> np.uint32(16)).astype(np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def _values(kind, n, k, storage="f32"):
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", 7 * n + k, (n, k))
    if storage == "bf16":                            # truncation keeps every special a special
        w = (np.ascontiguousarray(w).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return w


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


# ----------------------------------------------------------------------------- pack and unpack

@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_pack_transposed_bytes_equal_the_emulation_and_the_row_pack_of_a_copy(storage):
    for kind in ("heavy", "specials"):
        for n, k in NK:
            w = _values(kind, n, k, storage)
            wd = _dev(w, storage)
            wtd = _dev(np.ascontiguousarray(w.T), storage)          # a contiguous copy of Wᵀ
            for name, amap in _maps(n, k):
                want = packed.pack(np.ascontiguousarray(w.T), amap, backend="emulation")
                assert np.array_equal(packed.pack_transposed(w, amap).data, want.data)
                tables = hb.PackedTables.on_device(amap)
                got = hb.pack_tiles_transposed(wd, tables).cpu().numpy()
                again = hb.pack_tiles_transposed(wd, tables, out=torch.full((tables.nbytes,), 0xA5, dtype=torch.uint8, device="cuda"))
                rows = hb.pack_tiles(wtd, tables).cpu().numpy()
                assert got.size == want.nbytes == tables.nbytes
                diff = np.flatnonzero(got != want.data)
                assert diff.size == 0, (kind, n, k, name, storage, diff[:8])
                assert np.array_equal(got, rows), (kind, n, k, name, storage)
                assert np.array_equal(again.cpu().numpy(), got), (kind, n, k, name, storage)      # every byte written


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_pack_transposed_reads_rows_at_a_pitch(storage):
    w = _values("heavy", 70, 90, storage)
    full = _dev(w, storage)
    for c0, c1 in ((0, 50), (3, 53), (8, 72)):                              # ld > cols; aligned and unaligned first columns
        view = full[:, c0:c1]
        amap = random_map((c1 - c0, 70), 5)
        want = packed.pack(np.ascontiguousarray(w[:, c0:c1].T), amap, backend="emulation")
        got = hb.pack_tiles_transposed(view, hb.PackedTables.on_device(amap))
        assert np.array_equal(got.cpu().numpy(), want.data), (storage, c0, c1)
        pt = packed.pack_transposed(view, amap, backend="hip")              # the public entry reads the view in place too
        assert pt.shape == (c1 - c0, 70) and pt.layout == "rows" and np.array_equal(pt.data.cpu().numpy(), want.data)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_unpack_transposed_is_k3t_bit_for_bit(storage):
    for kind in ("heavy", "specials"):
        for n, k in NK:
            w = _values(kind, n, k, storage)
            wd = _dev(w, storage)
            for name, amap in _maps(n, k):
                tables = hb.PackedTables.on_device(amap)
                data = hb.pack_tiles_transposed(wd, tables)
                k3t = hb.apply_assignment_transposed(wd, np.asarray(amap)).cpu().numpy().view(np.uint32)
                y = hb.unpack_tiles_transposed(data, tables, n, k).cpu().numpy().view(np.uint32)
                assert y.shape == (n, k) and np.array_equal(y, k3t), (kind, n, k, name, storage, np.argwhere(y != k3t)[:4])
                assert np.array_equal(k3t, expected_bits(np.ascontiguousarray(w.T), amap).T), (kind, n, k, name)
                half = hb.unpack_tiles_transposed(data, tables, n, k, dtype=torch.bfloat16)
                h = half.view(torch.int16).cpu().numpy().view(np.uint16)
                assert np.array_equal(h, (k3t >> np.uint32(16)).astype(np.uint16)) and np.all(k3t & np.uint32(0xFFFF) == 0)
                for dtype in (torch.float32, torch.bfloat16):               # into a pitched output: only rows × cols is written
                    wide = torch.full((n + 2, k + 7), -1.0, dtype=dtype, device="cuda")
                    hb.unpack_tiles_transposed(data, tables, n, k, dtype=dtype, out=wide[1:1 + n, 3:3 + k])
                    full = wide.float().cpu().numpy()
                    inside = np.zeros(full.shape, dtype=bool)
                    inside[1:1 + n, 3:3 + k] = True
                    assert np.array_equal(full[1:1 + n, 3:3 + k].view(np.uint32), k3t) and np.all(full[~inside] == -1.0), (kind, n, k, name)


def test_the_public_interface_round_trips():
    w = _values("heavy", 72, 300)
    amap = random_map((300, 72), 9)
    pt = packed.pack_transposed(w, amap, backend="hip")
    assert pt.on_device and pt.shape == (300, 72) and pt.layout == "rows" and (pt.rows, pt.cols) == (300, 72)
    want = expected_bits(np.ascontiguousarray(w.T), amap)
    assert np.array_equal(packed.unpack_transposed(pt, backend="hip").cpu().numpy().view(np.uint32), want.T)
    assert np.array_equal(packed.unpack(pt, backend="hip").cpu().numpy().view(np.uint32), want)          # an ordinary row tensor of Wᵀ
    assert np.array_equal(np.asarray(packed.unpack_transposed(pt, backend="emulation")).view(np.uint32), want.T)
    half = packed.unpack_transposed(pt, backend="hip", dtype="bfloat16")
    assert half.dtype == torch.bfloat16 and np.array_equal(half.float().cpu().numpy().view(np.uint32), want.T)


# ----------------------------------------------------------------------------- the product

@functools.lru_cache(maxsize=None)
def _weights(n, k, kind, which):
    """(P̂ on the device, the all-bf16 row-layout packing of unpack(P̂)ᵀ, bias) — made once, never written to.  The unpacked matrix comes
    from the NumPy decoder on the device's bytes, not from the new unpack kernel."""
    w = _values(kind, n, k)
    amap = next(a for name, a in _maps(n, k) if name == which)
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


def _into_sentinels(xd, pt, tables, n, bias, dtype):
    """hb.packed_matmul into a pitched view of a buffer of sentinels → the (m, n) result; the columns and rows around it stay."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_matmul(xd, pt.data, tables, n, bias=bias, out_dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = buf.float().cpu().numpy()
    inside = np.zeros(whole.shape, dtype=bool)
    inside[1:1 + m, 2:2 + n] = True
    assert np.all(whole[~inside] == sentinel), (m, n, np.argwhere((whole != sentinel) & ~inside)[:4])
    return out


def _bit_contract(m, n, k, kind, names):
    plain, pitched = _x(m, k)
    for which in names:
        pt, ref, bd = _weights(n, k, kind, which)
        for layout, xd in (("contiguous", plain), ("pitched", pitched)):
            for out_dtype, dtype in DTYPES:
                for bias in (None, bd):
                    what = (m, n, k, kind, which, layout, out_dtype, bias is not None)
                    want = packed.linear(xd, ref, bias=bias, out_dtype=out_dtype, kernel="block")
                    got = packed.matmul(xd, pt, bias=bias, out_dtype=out_dtype)
                    assert got.dtype == dtype and tuple(got.shape) == (m, n)
                    _same(got, want, kind == "specials", what)
                    _same(packed.matmul(xd, pt, bias=bias, out_dtype=out_dtype), got, kind == "specials", what + ("again",))
                    _same(_into_sentinels(xd, pt, pt.tables(), n, bias, dtype), want, kind == "specials", what + ("pitched y",))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_matmul_is_the_block_kernel_on_the_transposed_weight_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy", ("random", "bfp4", "bf16"))
    if k <= 320:
        _bit_contract(m, n, k, "specials", ("random",))


@pytest.mark.parametrize("m", [1, 33, 130])
def test_matmul_integer_grid_is_exact(m):
    for n in (40, 72, 200):
        for k in (100, 300):
            x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
            for _name, amap in _maps(n, k):
                phat = _phat(w, amap)                                       # (k, n)
                _grid_preconditions(x, phat.T, b.astype(np.float64))
                want = x.astype(np.float64) @ phat + b.astype(np.float64)[None, :]
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
                pt = packed.pack_transposed(w, amap, backend="hip")
                bd = torch.from_numpy(b).cuda()
                got = packed.matmul(_x_dev(x), pt, bias=bd).cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, _name, np.argwhere(got != want)[:4])
                nob = packed.matmul(_x_dev(x), pt).cpu().numpy()
                assert np.array_equal(nob.astype(np.float64), want - b.astype(np.float64)[None, :]), (m, n, k, _name)
                yb = packed.matmul(_x_dev(x), pt, bias=bd, out_dtype="bfloat16")
                assert np.array_equal(yb.float().cpu().numpy(), torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16).float().numpy())


def _one_hot_mismatches(n, k, s, seed, corrupt=False):
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((k, n), seed + 1).copy()
    amap[0, 0] = 1
    pt = packed.pack_transposed(w, amap, backend="hip")
    if corrupt:     # one code byte of tile 0 (bfp8): element (row 0, column 5) of P̂ changes its last mantissa bit
        pt.data[int(pt.offsets[0]) * 64 + 64 + 5] ^= 0x01
    x = (np.eye(k, dtype=np.float32) * np.float32(2.0 ** s))
    y = packed.matmul(_x_dev(x), pt).cpu().numpy().astype(np.float64)
    want = (2.0 ** s) * _phat(w, amap)
    assert y.shape == want.shape == (k, n)
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return np.argwhere(y != want)


@pytest.mark.parametrize("n,k,s", [(70, 160, 3), (64, 64, -2), (200, 100, 0), (40, 300, 1)])
def test_matmul_one_hot_pins_every_position(n, k, s):
    bad = _one_hot_mismatches(n, k, s, 50 + n)
    assert bad.size == 0, bad[:8]


def test_matmul_one_hot_fails_on_a_wrong_image():
    bad = _one_hot_mismatches(70, 160, 3, 120, corrupt=True)
    assert [tuple(r) for r in bad] == [(0, 5)]          # Y[k = 0, n = 5] alone


@pytest.mark.parametrize("m,n,k", [(1, 72, 100), (33, 200, 300), (130, 40, 100), (130, 72, 320)])
def test_matmul_random_is_within_the_f32_accumulation_bound(m, n, k):
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
    emu = packed.matmul(x, packed.pack_transposed(w, amap), bias=b, backend="emulation")
    assert np.array_equal(emu, want.astype(np.float32))                     # the emulation is this float64 expression, rounded once
    for xd in (_x_dev(x), wide[:, 1:1 + k]):
        got = packed.matmul(xd, pt, bias=bd).cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print(f"m={m} n={n} k={k}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), (m, n, k, float(np.max(err / np.maximum(bound, 1e-300))))
        yb = packed.matmul(xd, pt, bias=bd, out_dtype="bfloat16")
        errb = np.abs(yb.float().cpu().numpy().astype(np.float64) - want)
        assert np.all(errb <= bound * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want)), (m, n, k)


# ----------------------------------------------------------------------------- guards and boundaries

@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 33, 200, 100                                # P̂'s grid 4 × 7
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
    """mtq_packed_matmul through `tables`, with and without bias, against the exact product with `phat_left`.  pt.data is the whole
    stream: a kernel without the guard reads real bytes and the comparison fails."""
    assert pt.data.numel() == pt.nbytes == pt.tables().nbytes                # never a shorter buffer
    b64 = b.astype(np.float64)
    nob_want = x.astype(np.float64) @ phat_left
    assert np.array_equal(nob_want.astype(np.float32).astype(np.float64), nob_want)
    bd = torch.from_numpy(b.copy()).cuda()
    got = hb.packed_matmul(_x_dev(x), pt.data, tables, n, bias=bd).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, nob_want + b64[None, :]), np.argwhere(got != nob_want + b64[None, :])[:4]
    nob = hb.packed_matmul(_x_dev(x), pt.data, tables, n).cpu().numpy().astype(np.float64)
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
    t_a, t_b = 0 * tiles_w + 3, 2 * tiles_w + 4                              # K steps 0 and 1, column blocks 1 and 2
    tables.map_dev[t_a] = 4
    tables.map_dev[t_b] = -1
    left = _zeroed(phat, tiles_w, (t_a, t_b))
    assert 0 < np.count_nonzero(left != phat) <= 2 * 32 * 32
    _guarded_outputs_equal(x, pt, tables, n, b, left)
    assert np.array_equal(pt.tables().map_dev.cpu().numpy(), pt.map.reshape(-1))                 # the shared tables were not touched


def test_boundaries_and_the_module():
    w = _values("heavy", 72, 100)
    amap = random_map((100, 72), 3)
    pt = packed.pack_transposed(w, amap, backend="hip")
    for out_dtype, dtype in DTYPES:
        empty = packed.matmul(torch.zeros((0, 100), dtype=torch.bfloat16, device="cuda"), pt, out_dtype=out_dtype)
        assert tuple(empty.shape) == (0, 72) and empty.dtype == dtype
    x = to_bf16_valued(gen("normal_f32", 5, (2, 3, 100)))
    bias = gen("normal_f32", 6, (72,))
    mod = packed.PackedMatmul(pt, bias=bias, out_dtype="bfloat16")
    assert mod.backend == "hip" and (mod.in_features, mod.out_features) == (100, 72)
    y = mod(_x_dev(x))
    want = packed.matmul(_x_dev(x.reshape(6, 100)), pt, bias=torch.from_numpy(bias).cuda(), out_dtype="bfloat16")
    assert tuple(y.shape) == (2, 3, 72) and torch.equal(y.reshape(6, 72).view(torch.int16), want.view(torch.int16))
    assert tuple(mod(torch.zeros((0, 100), dtype=torch.bfloat16, device="cuda")).shape) == (0, 72)
    for n, k in ((1, 100), (72, 1), (1, 1)):             # one column, one k-row
        xg, wg, bg = _grid_case(33, n, k, 77 + n + k)
        a = random_map((k, n), n + k)
        phat = _phat(wg, a)
        _grid_preconditions(xg, phat.T, bg.astype(np.float64))
        got = packed.matmul(_x_dev(xg), packed.pack_transposed(wg, a, backend="hip"), bias=torch.from_numpy(bg).cuda()).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), xg.astype(np.float64) @ phat + bg.astype(np.float64)[None, :]), (n, k)
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.packed_matmul(_x_dev(x.reshape(6, 100)), pt.data, pt.tables(), 20)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_matmul(_x_dev(x.reshape(6, 100)).float(), pt.data, pt.tables(), 72)
