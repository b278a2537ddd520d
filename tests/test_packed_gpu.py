"""GPU: the packed mixed-tile kernels (csrc/mtq_packed.hip) against the NumPy encoder of quantization_analysis_amd/packed.py, K3 and
exact arithmetic.

  * pack: the device stream is the emulation's stream byte for byte (bf16 and float32 storage, ragged edges, a row pitch, specials),
    and two runs give the same bytes;
  * unpack: float32 y is K3's y (mtq_apply_assignment) bit for bit, bf16 y its upper halves;
  * linear, exact (the style of test_output_error_exact_gpu.py):
      integer grid — X integers |x| ≤ 4, W and the bias on the 2⁻⁸ grid with |w| < 1: Ŵ stays on the grid and every partial sum below
        2²⁴ grid units (asserted on the host for every case), so f32 accumulation is exact in any order and Y must EQUAL the float64
        X·Ŵᵀ + b;
      one-hot — m = k, row i of X is 2ˢ·e_i: Y[i, j] = 2ˢ·Ŵ[j, i] exactly, which pins the decode of every (n, k) position of every
        format under a random map; flipping one code byte of the stream must show;
  * linear, random: |Y − Y₆₄| ≤ (k + 2)·2⁻²⁴·(Σ_k |x||ŵ| + |b|) — k products are exact, k − 1 f32 additions of the accumulator, one for
    the bias and one spare, each with relative error 2⁻²⁴ of a partial sum that Σ|x||ŵ| + |b| bounds; a bf16 Y adds a relative 2⁻⁸.
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


def dev(x: np.ndarray, storage: str):
    """float32 values → device tensor; bf16 storage takes the upper halves of the words (the values must be bf16-valued)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    if storage == "f32":
        return torch.from_numpy(u.view(np.float32).copy()).cuda()
    assert np.all(u & np.uint32(0xFFFF) == 0)
    return torch.from_numpy((u >> np.uint32(16)).astype(np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def bf16_valued_bits(x: np.ndarray) -> np.ndarray:
    """Truncate the words to bf16 (keeps every special a special)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, float32 values, map) — computed once, shared, never written to."""
    out = []
    for code in range(4):
        out.append((f"32x32-{hb.MIXED_TILE_FORMATS[code]}", gen("heavy_f32", 20 + code, (32, 32)), uniform_map((32, 32), code)))
    out.append(("96x160-random", gen("heavy_f32", 31, (96, 160)), random_map((96, 160), 1)))
    out.append(("70x50-ragged", gen("normal_f32", 32, (70, 50)), random_map((70, 50), 2)))
    out.append(("70x50-specials", specials((70, 50)), random_map((70, 50), 3)))
    out.append(("96x160-specials", specials((96, 160), seed=5), random_map((96, 160), 4)))
    for _n, x, _a in out:
        x.setflags(write=False)
    return out


def _storage_values(x, storage):
    return x if storage == "f32" else bf16_valued_bits(x)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_pack_bytes_equal_the_emulation(storage):
    for name, x, amap in cases():
        xv = _storage_values(x, storage)
        want = packed.pack(xv, amap, backend="emulation")
        xd = dev(xv, storage)
        tables = hb.PackedTables.on_device(amap)
        got = hb.pack_tiles(xd, tables)
        again = hb.pack_tiles(xd, tables, out=torch.full((tables.nbytes,), 0xA5, dtype=torch.uint8, device="cuda"))
        g = got.cpu().numpy()
        assert g.size == want.nbytes == tables.nbytes
        diff = np.flatnonzero(g != want.data)
        assert diff.size == 0, (name, storage, diff[:8], g[diff[:8]], want.data[diff[:8]])
        assert np.array_equal(again.cpu().numpy(), g), (name, storage)      # every byte written, the same bytes


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_pack_reads_rows_at_a_pitch(storage):
    x = gen("heavy_f32", 41, (70, 90))
    xv = _storage_values(x, storage)
    full = dev(xv, storage)
    for c0, c1 in ((0, 50), (3, 53), (8, 72)):                              # ld > cols; aligned and unaligned first columns
        view = full[:, c0:c1]
        amap = random_map((70, c1 - c0), 5)
        want = packed.pack(xv[:, c0:c1], amap, backend="emulation")
        got = hb.pack_tiles(view, hb.PackedTables.on_device(amap))
        assert np.array_equal(got.cpu().numpy(), want.data), (storage, c0, c1)


def test_pack_through_the_public_interface():
    for shape in ((100,), (), (3, 40, 64)):
        x = gen("heavy_f32", 7, shape)
        amap = random_map(orc.flatten_2d(x)[0].shape, 6)
        pt = packed.pack(x, amap, backend="hip")
        want = packed.pack(x, amap, backend="emulation")
        assert pt.on_device and np.array_equal(pt.data.cpu().numpy(), want.data) and np.array_equal(pt.offsets, want.offsets)
        y = packed.unpack(pt, backend="hip")
        assert tuple(y.shape) == tuple(shape)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), expected_bits(x, amap))
        assert np.array_equal(np.asarray(packed.unpack(pt, backend="emulation")).view(np.uint32), expected_bits(x, amap))


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_unpack_is_k3_bit_for_bit(storage):
    for name, x, amap in cases():
        xv = _storage_values(x, storage)
        xd = dev(xv, storage)
        tables = hb.PackedTables.on_device(amap)
        data = hb.pack_tiles(xd, tables)
        rows, cols = xv.shape
        k3 = hb.apply_assignment(xd, np.asarray(amap)).cpu().numpy().view(np.uint32)
        y = hb.unpack_tiles(data, tables, rows, cols).cpu().numpy().view(np.uint32)
        assert np.array_equal(y, k3), (name, storage, np.argwhere(y != k3)[:4])
        assert np.array_equal(k3, expected_bits(xv, amap)), name
        half = hb.unpack_tiles(data, tables, rows, cols, dtype=torch.bfloat16)
        h = half.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(h, (k3 >> np.uint32(16)).astype(np.uint16)) and np.all(k3 & np.uint32(0xFFFF) == 0), (name, storage)
        # into a pitched output: only rows × cols is written
        wide = torch.full((rows, cols + 7), -1.0, dtype=torch.float32, device="cuda")
        hb.unpack_tiles(data, tables, rows, cols, out=wide[:, 3:3 + cols])
        w = wide.cpu().numpy()
        assert np.array_equal(w[:, 3:3 + cols].view(np.uint32), k3) and np.all(w[:, :3] == -1.0) and np.all(w[:, 3 + cols:] == -1.0)


# ----------------------------------------------------------------------------- linear


def _what(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """Ŵ as float64, from the oracle."""
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(x).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("m", [1, 33, 133])
def test_linear_integer_grid_is_exact(m):
    for n in (64, 70):
        for k in (64, 100, 160):
            x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
            for amap in (random_map((n, k), m + n + k), uniform_map((n, k), 2)):
                what = _what(w, amap)
                _grid_preconditions(x, what, b.astype(np.float64))
                want = x.astype(np.float64) @ what.T + b.astype(np.float64)[None, :]
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
                pt = packed.pack(w, amap, backend="hip")
                y = packed.linear(_x_dev(x), pt, bias=torch.from_numpy(b).cuda())
                got = y.cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, np.argwhere(got != want)[:4])
                nob = packed.linear(_x_dev(x), pt).cpu().numpy()
                assert np.array_equal(nob.astype(np.float64), want - b.astype(np.float64)[None, :]), (m, n, k)
                yb = packed.linear(_x_dev(x), pt, bias=torch.from_numpy(b).cuda(), out_dtype="bfloat16")
                assert np.array_equal(yb.float().cpu().numpy(), torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16).float().numpy())


def _one_hot_mismatches(n, k, s, seed, corrupt=False):
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((n, k), seed + 1).copy()
    amap[0, 0] = 1
    pt = packed.pack(w, amap, backend="hip")
    if corrupt:     # one code byte of tile 0 (bfp8): element (row 0, column 5) changes its last mantissa bit
        pt.data[int(pt.offsets[0]) * 64 + 64 + 5] ^= 0x01
    x = (np.eye(k, dtype=np.float32) * np.float32(2.0 ** s))
    y = packed.linear(_x_dev(x), pt).cpu().numpy().astype(np.float64)
    want = (2.0 ** s) * _what(w, amap).T
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return np.argwhere(y != want)


@pytest.mark.parametrize("n,k,s", [(70, 160, 3), (64, 64, -2), (130, 100, 0)])
def test_linear_one_hot_pins_every_position(n, k, s):
    bad = _one_hot_mismatches(n, k, s, 50 + n)
    assert bad.size == 0, bad[:8]


def test_linear_one_hot_fails_on_a_wrong_image():
    bad = _one_hot_mismatches(70, 160, 3, 120, corrupt=True)
    assert [tuple(r) for r in bad] == [(5, 0)]          # Y[k = 5, n = 0] alone


@pytest.mark.parametrize("m,n,k", [(1, 70, 100), (33, 130, 200), (133, 70, 100), (130, 64, 72)])
def test_linear_random_is_within_the_f32_accumulation_bound(m, n, k):
    w = gen("heavy_f32", 60 + m, (n, k))
    x = to_bf16_valued(gen("normal_f32", 61 + m, (m, k)) * 40)
    b = gen("normal_f32", 62 + m, (n,))
    amap = random_map((n, k), 63 + m)
    what = _what(w, amap)
    want = x.astype(np.float64) @ what.T + b.astype(np.float64)[None, :]
    bound = (k + 2) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(what).T + np.abs(b).astype(np.float64)[None, :])
    pt = packed.pack(w, amap, backend="hip")
    bd = torch.from_numpy(b).cuda()
    # X at a row pitch with an unaligned first element: the scalar load path; and contiguous: the vector path
    wide = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    wide[:, 1:1 + k] = _x_dev(x)
    for xd in (_x_dev(x), wide[:, 1:1 + k]):
        y = packed.linear(xd, pt, bias=bd)
        again = packed.linear(xd, pt, bias=bd)
        got = y.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print(f"m={m} n={n} k={k}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), (m, n, k, float(np.max(err / np.maximum(bound, 1e-300))))
        assert torch.equal(y.view(torch.int32), again.view(torch.int32))
        yb = packed.linear(xd, pt, bias=bd, out_dtype="bfloat16")
        errb = np.abs(yb.float().cpu().numpy().astype(np.float64) - want)
        assert np.all(errb <= bound * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want)), (m, n, k)
        assert torch.equal(yb.view(torch.int16), packed.linear(xd, pt, bias=bd, out_dtype="bfloat16").view(torch.int16))


def test_linear_from_a_loaded_file_and_refusals(tmp_path):
    w = gen("heavy_bf16", 70, (70, 100))
    amap = random_map((70, 100), 71)
    host = packed.pack(w, amap, backend="emulation")
    packed.save(tmp_path / "w.npz", host)
    pt = packed.load(tmp_path / "w.npz")
    x = to_bf16_valued(gen("normal_f32", 72, (5, 100)))
    y = packed.linear(_x_dev(x), pt, backend="hip").cpu().numpy()           # the stream moves to the device on first use
    assert pt.on_device
    want = packed.linear(x, host, backend="emulation")
    assert np.allclose(y, want, rtol=0, atol=float(np.max(102 * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(_what(w, amap)).T))))
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.packed_linear(_x_dev(x), pt.data, pt.tables(), 64)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_linear(_x_dev(x).float(), pt.data, pt.tables(), 70)
