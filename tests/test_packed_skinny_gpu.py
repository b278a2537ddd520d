"""GPU: the skinny packed linear (packed_linear_skinny_kernel, m <= 32, split over K) held to what tests/test_packed_gpu.py holds the
block kernel to, at the smallest shapes that reach every branch: a ragged last tile row (n = 70), a ragged last tile column and 2, 4
and 5 tile columns (k = 64, 100, 160: uneven slices), m on both sides of 16 and at 32, every split route (the library's choice, 1 =
direct, 2, 5, and 9 > tiles_w), random maps over all four codes and the four uniform maps.

  * integer grid (the construction and precondition asserts of test_linear_integer_grid_is_exact: every order is exact): Y EQUALS the
    float64 product with and without bias, the bf16 Y is the once-rounded float32 Y, and Y is the block kernel's Y bit for bit;
  * one-hot: X = rows [32c, 32c + 32) of 2ˢ·I_k, one call per c: the assembled k × n result is 2ˢ·Ŵᵀ from the oracle at every position,
    at split 1 and at a forced split; one flipped code byte shows at exactly its position;
  * random: |Y − Y₆₄| ≤ (k + 2)·2⁻²⁴·(Σ|x||ŵ| + |b|), the block kernel's bound (it holds for any order); X and Y at row pitches;
    two calls, a call on a workspace full of 0xFF and a call on another call's workspace give the same bits;
  * the kernel's own decode (a cheaper form of the block kernel's) gives bfp_code_bits_rt's word for every exponent byte, every code
    and every position of the group, in all three formats, and those words are the NumPy decoder's;
  * routing: "skinny" refuses m = 33, "auto" is one of the two kernels bit for bit, PackedLinear is packed.linear on the flatten.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import GRID, expected_bits, random_map, uniform_map

pytestmark = pytest.mark.gpu
SPLITS = (0, 1, 2, 5, 9)
MAPS = ("random", "0", "1", "2", "3")


def _what(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """Ŵ as float64, from the oracle."""
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _bits(t) -> np.ndarray:
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _grid_weight(n, k, which):
    """(packed weight on the device, Ŵ float64, bias float32) on the 2⁻⁸ grid — computed once per (n, k, map), never written to."""
    rng = np.random.default_rng(10 * n + k)
    w = (rng.integers(-255, 256, size=(n, k)) * GRID).astype(np.float32)
    b = (rng.integers(-255, 256, size=(n,)) * GRID).astype(np.float32)
    amap = random_map((n, k), n + k) if which == "random" else uniform_map((n, k), int(which))
    what = _what(w, amap)
    assert np.array_equal(what / GRID, np.round(what / GRID)) and np.array_equal(b / GRID, np.round(b / GRID))
    what.setflags(write=False)
    b.setflags(write=False)
    return packed.pack(w, amap, backend="hip"), what, b


def grid_case_is_exact(m, n, k, splits=SPLITS, maps=MAPS):
    """The integer-grid case (m, n, k) under every map of `maps` and every split of `splits` (tests/test_packed_long_k_gpu.py runs it
    at long K)."""
    x = np.random.default_rng(1000 * m + 10 * n + k).integers(-4, 5, size=(m, k)).astype(np.float32)
    assert np.all(np.abs(x) <= 4) and np.array_equal(x, np.round(x))
    xd = _x_dev(x)
    for which in maps:
        pt, what, b = _grid_weight(n, k, which)
        b64 = b.astype(np.float64)
        worst = (np.abs(x).astype(np.float64) @ np.abs(what).T + np.abs(b64)[None, :]) / GRID
        assert worst.max() < 2.0 ** 24                             # every partial sum is exact in f32, in any order
        want = x.astype(np.float64) @ what.T + b64[None, :]
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        bd = torch.from_numpy(b.copy()).cuda()
        block = packed.linear(xd, pt, bias=bd)
        block_nob = packed.linear(xd, pt)
        want_bf16 = torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)
        for split in splits:
            y = packed.linear(xd, pt, bias=bd, kernel="skinny", split=split)
            got = y.cpu().numpy()
            assert got.shape == (m, n) and got.dtype == np.float32
            assert np.array_equal(got.astype(np.float64), want), (m, n, k, which, split, np.argwhere(got != want)[:4])
            nob = packed.linear(xd, pt, kernel="skinny", split=split)
            assert np.array_equal(nob.cpu().numpy().astype(np.float64), want - b64[None, :]), (m, n, k, which, split)
            yb = packed.linear(xd, pt, bias=bd, kernel="skinny", split=split, out_dtype="bfloat16")
            assert yb.dtype == torch.bfloat16 and np.array_equal(_bits(yb), _bits(want_bf16)), (m, n, k, which, split)
            assert np.array_equal(_bits(y), _bits(block)) and np.array_equal(_bits(nob), _bits(block_nob)), (m, n, k, which, split)


@pytest.mark.parametrize("m", [1, 5, 16, 17, 32])
def test_skinny_integer_grid_is_exact(m):
    for n in (64, 70):
        for k in (64, 100, 160):
            grid_case_is_exact(m, n, k)


def _one_hot_mismatches(n, k, s, seed, split, corrupt=False):
    w = gen("heavy_f32", seed, (n, k))
    amap = random_map((n, k), seed + 1).copy()
    amap[0, 0] = 1
    pt = packed.pack(w, amap, backend="hip")
    if corrupt:     # one code byte of tile 0 (bfp8): element (row 0, column 5) changes its last mantissa bit
        pt.data[int(pt.offsets[0]) * 64 + 64 + 5] ^= 0x01
    eye = np.eye(k, dtype=np.float32) * np.float32(2.0 ** s)
    rows = [packed.linear(_x_dev(eye[c:c + 32]), pt, kernel="skinny", split=split) for c in range(0, k, 32)]
    y = torch.cat(rows).cpu().numpy().astype(np.float64)
    want = (2.0 ** s) * _what(w, amap).T
    assert y.shape == want.shape == (k, n)
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return np.argwhere(y != want)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("n,k,s", [(70, 160, 3), (64, 64, -2), (130, 100, 0)])
def test_skinny_one_hot_pins_every_position(n, k, s, split):
    bad = _one_hot_mismatches(n, k, s, 50 + n, split)
    assert bad.size == 0, bad[:8]


@pytest.mark.parametrize("split", [1, 3])
def test_skinny_one_hot_fails_on_a_wrong_image(split):
    bad = _one_hot_mismatches(70, 160, 3, 120, split, corrupt=True)
    assert [tuple(r) for r in bad] == [(5, 0)]          # Y[k = 5, n = 0] alone


def random_case_is_within_the_bound(m, n, k):
    """Random values at (m, n, k): the bound, both X layouts, splits 0, 1 and 3, repeatability, the workspace's contents, a pitched Y."""
    w = gen("heavy_f32", 60 + m, (n, k))
    x = to_bf16_valued(gen("normal_f32", 61 + m, (m, k)) * 40)
    b = gen("normal_f32", 62 + m, (n,))
    amap = random_map((n, k), 63 + m)
    what = _what(w, amap)
    want = x.astype(np.float64) @ what.T + b.astype(np.float64)[None, :]
    bound = (k + 2) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(what).T + np.abs(b).astype(np.float64)[None, :])
    pt = packed.pack(w, amap, backend="hip")
    tables = pt.tables()
    bd = torch.from_numpy(b).cuda()
    # X at a row pitch with an unaligned first element: the scalar load path; and contiguous: the vector path
    wide = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    wide[:, 1:1 + k] = _x_dev(x)
    other_m = 5 if m != 5 else 7
    for xd in (_x_dev(x), wide[:, 1:1 + k]):
        for split in (0, 1, 3):
            y = packed.linear(xd, pt, bias=bd, kernel="skinny", split=split)
            got = y.cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            print(f"m={m} n={n} k={k} split={split}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound), (m, n, k, split, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.array_equal(_bits(packed.linear(xd, pt, bias=bd, kernel="skinny", split=split)), _bits(y))
            yb = packed.linear(xd, pt, bias=bd, kernel="skinny", split=split, out_dtype="bfloat16")
            errb = np.abs(yb.float().cpu().numpy().astype(np.float64) - want)
            assert np.all(errb <= bound * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want)), (m, n, k, split)
            assert np.array_equal(_bits(yb), _bits(y.to(torch.bfloat16)))                   # one rounding of the float32 result
            # an output at a row pitch: only m × n is written
            frame = torch.full((m, n + 7), -1.0, dtype=torch.float32, device="cuda")
            hb.packed_linear_skinny(xd, pt.data, tables, n, bias=bd, out=frame[:, 3:3 + n], split=split)
            f = frame.cpu().numpy()
            assert np.array_equal(f[:, 3:3 + n].view(np.int32), _bits(y)) and np.all(f[:, :3] == -1.0) and np.all(f[:, 3 + n:] == -1.0)
            # the workspace's contents on entry mean nothing: 0xFF bytes, then what a call with another (m, split) left there
            need = max(hb.packed_linear_skinny_workspace_bytes(mm, n, k, sp) for mm in (m, other_m) for sp in (split, 2))
            ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
            assert np.array_equal(_bits(hb.packed_linear_skinny(xd, pt.data, tables, n, bias=bd, split=split, workspace=ws)), _bits(y))
            hb.packed_linear_skinny(xd[:1].expand(other_m, k).contiguous(), pt.data, tables, n, split=2, workspace=ws)
            assert np.array_equal(_bits(hb.packed_linear_skinny(xd, pt.data, tables, n, bias=bd, split=split, workspace=ws)), _bits(y))
    with pytest.raises(hb.MtqError, match="workspace"):
        hb.packed_linear_skinny(_x_dev(x), pt.data, tables, n, split=2, workspace=torch.empty(15, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("m,n,k", [(1, 70, 100), (17, 130, 200), (32, 70, 160)])
def test_skinny_random_is_within_the_f32_accumulation_bound(m, n, k):
    random_case_is_within_the_bound(m, n, k)


@pytest.mark.parametrize("fmt,mant", [("bfp8", 7), ("bfp4", 3), ("bfp2", 1)])
def test_skinny_decode_is_the_reference_decode_for_every_exponent_and_code(fmt, mant):
    got, want = (t.cpu().numpy().view(np.uint32) for t in hb.debug_packed_decode(fmt))
    assert got.shape == want.shape == (16, 256, 16, 16)
    rot, E, q, i = np.ogrid[:16, :256, :16, :16]
    codes = ((16 * q + (i + rot) % 16) % (1 << (mant + 1))).astype(np.uint8) + np.zeros_like(E, dtype=np.uint8)
    assert set(np.unique(codes)) == set(range(1 << (mant + 1)))                          # every code, at every position (rot)
    host = packed.decode_groups(np.broadcast_to(E[..., 0], codes.shape[:3]).astype(np.uint8), codes, mant)
    assert np.array_equal(want, host)                                                    # the device reference is the format's decode
    bad = np.argwhere(got != want)
    assert bad.size == 0, (fmt, bad[:8], got[tuple(bad[0])] if bad.size else None)
    assert np.all(got & np.uint32(0xFFFF) == 0)                                          # bf16-valued: the MFMA operand drops nothing


def test_routing_and_the_module():
    n, k = 70, 160
    w = gen("heavy_f32", 80, (n, k))
    pt = packed.pack(w, random_map((n, k), 81), backend="hip")
    bd = torch.from_numpy(gen("normal_f32", 82, (n,))).cuda()
    x33 = _x_dev(to_bf16_valued(gen("normal_f32", 83, (33, k))))
    with pytest.raises(hb.MtqError, match="m <= 32"):
        packed.linear(x33, pt, kernel="skinny")
    with pytest.raises(hb.MtqError, match="m <= 32"):
        hb.packed_linear_skinny(x33, pt.data, pt.tables(), n)
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.linear(x33, pt, kernel="nonsense")
    assert np.array_equal(_bits(packed.linear(x33, pt, bias=bd, kernel="auto")), _bits(packed.linear(x33, pt, bias=bd, kernel="block")))
    assert np.array_equal(_bits(packed.linear(x33, pt, bias=bd)), _bits(packed.linear(x33, pt, bias=bd, kernel="block")))   # the default
    for m in (1, 6, 16, 32):
        auto = _bits(packed.linear(x33[:m], pt, bias=bd, kernel="auto"))
        skinny, block = (_bits(packed.linear(x33[:m], pt, bias=bd, kernel=name)) for name in ("skinny", "block"))
        assert np.array_equal(auto, skinny if m <= packed.AUTO_SKINNY_MAX_M else block), m
    for out_dtype in ("float32", "bfloat16"):
        layer = packed.PackedLinear(pt, bias=bd, out_dtype=out_dtype)
        assert layer.backend == "hip" and layer.kernel == "auto"
        x3 = x33[:6].reshape(2, 3, k)
        y = layer(x3)
        assert tuple(y.shape) == (2, 3, n) and y.is_cuda and not y.requires_grad
        assert np.array_equal(_bits(y.reshape(6, n)), _bits(packed.linear(x33[:6], pt, bias=bd, out_dtype=out_dtype, kernel="auto")))
        assert np.array_equal(_bits(layer(x3)), _bits(y))                                   # k = 160 needs no workspace: test_packed_long_k_gpu.py has a kept one
        big = layer(x33)                                                                     # m = 33: the block kernel
        assert np.array_equal(_bits(big), _bits(packed.linear(x33, pt, bias=bd, out_dtype=out_dtype)))
