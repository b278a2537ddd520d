"""GPU: the wide block with a split over K — packed_wide_split_kernel of csrc/mtq_packed.hip (wide_block over one K slice, f32 partials) and
skinny_reduce_kernel behind it — through packed.linear_wide / matmul_wide(split=), PackedLinear / PackedMatmul(wide_split=).

The block is 128 (M) × 128 (N), a step 64 of K, a slice whole steps [s·steps / S, (s + 1)·steps / S).  The shapes, with their steps:

  (1, 70, 64)      1 step: every split is 1, the wide kernel itself;
  (33, 129, 200)   4 steps, the last ragged; k % 8 == 0 (the 16-byte X loads); a second column block of one column;
  (130, 70, 320)   5 steps: 2 + 3 and 1 + 2 + 2, one-step slices at split 5; a second row block of two rows;
  (64, 128, 449)   8 steps in 3 (2 + 3 + 3), k % 8 != 0 (the element-wise X loads) with a one-column last step; whole blocks.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import _grid_case, _grid_preconditions, expected_bits, random_map, specials, uniform_map

pytestmark = pytest.mark.gpu
SHAPES = ((1, 70, 64), (33, 129, 200), (130, 70, 320), (64, 128, 449))
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def _steps(k):
    return -(-k // 64)


def _bits(t) -> np.ndarray:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(got, want, what):
    """Equal words; NaNs by position."""
    gn, wn = torch.isnan(got).cpu().numpy(), torch.isnan(want).cpu().numpy()
    assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:4])
    g, w = np.where(gn, 0, _bits(got)), np.where(wn, 0, _bits(want))
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:4])


@functools.lru_cache(maxsize=None)
def _grid(m, n, k):
    """The integer grid under random maps, both orientations: (x on the device, bias on the device, ((fn, pt, float64 want), ...)) — made
    once, never written to.  Every product is a multiple of 2^-8 and every sum of them stays below 2^24 of those: each partial and each
    sum of partials is exact in float32, so the result is the float64 product at every split."""
    x, w, b = _grid_case(m, n, k, 1000 * m + 10 * n + k)
    b64, out = b.astype(np.float64), []
    a_nk, a_kn = random_map((n, k), n + k), random_map((k, n), n + k + 1)
    for fn, pt, what in ((packed.linear_wide, packed.pack(w, a_nk, backend="hip"), expected_bits(w, a_nk)),                           # Ŵ (n, k)
                         (packed.matmul_wide, packed.pack_transposed(w, a_kn, backend="hip"), expected_bits(np.ascontiguousarray(w.T), a_kn).T)):
        what = what.view(np.float32).astype(np.float64)
        _grid_preconditions(x, what, b64)
        want = x.astype(np.float64) @ what.T
        assert np.array_equal((want + b64).astype(np.float32).astype(np.float64), want + b64)
        out.append((fn, pt, want))
    return torch.from_numpy(x).to(torch.bfloat16).cuda(), torch.from_numpy(b).cuda(), b64, tuple(out)


@pytest.mark.parametrize("split", (0, 1, 2, 3, "steps", "steps + 1"))
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_the_integer_grid_is_the_float64_product_at_every_split(m, n, k, split):
    split = {"steps": _steps(k), "steps + 1": _steps(k) + 1}.get(split, split)
    xd, bd, b64, cases = _grid(m, n, k)
    for fn, pt, want in cases:
        for bias, add in ((None, 0.0), (bd, b64[None, :])):
            got = fn(xd, pt, bias=bias, split=split)
            assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().astype(np.float64), want + add), \
                (fn.__name__, split, np.argwhere(got.cpu().numpy() != want + add)[:4])
            got = fn(xd, pt, bias=bias, split=split, out_dtype="bfloat16")
            assert np.array_equal(_bits(got), _bits(torch.from_numpy((want + add).astype(np.float32)).to(torch.bfloat16))), (fn.__name__, split)


@functools.lru_cache(maxsize=None)
def _inexact(m, n, k, kn, kind="specials"):
    """specials (Inf, NaN, denormals) or heavy-tailed weights under a random map, bf16 X, a bias; P the (n, k) bf16 words the kernel
    multiplies with (unpack, exact)."""
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", 7 * n + k, (n, k))
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 40)).to(torch.bfloat16).cuda()
    bias = torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda()
    if kn:
        pt = packed.pack_transposed(w, random_map((k, n), n + k), backend="hip")
        return x, bias, pt, packed.unpack(pt, backend="hip", dtype="bfloat16").t().contiguous()
    pt = packed.pack(w, random_map((n, k), n + k), backend="hip")
    return x, bias, pt, packed.unpack(pt, backend="hip", dtype="bfloat16")


@pytest.mark.parametrize("kind", ("specials", "heavy"))
@pytest.mark.parametrize("m,n,k,kn", ((33, 129, 200, False), (130, 70, 320, False), (33, 129, 200, True)))
def test_a_split_is_the_slices_summed_in_ascending_order(m, n, k, kn, kind):
    x, bias, pt, p = _inexact(m, n, k, kn, kind)
    fn, steps = (packed.matmul_wide if kn else packed.linear_wide), _steps(k)
    for out_dtype, dtype in DTYPES:
        for b in (None, bias):
            _same(fn(x, pt, bias=b, out_dtype=out_dtype, split=1, workspace=None), fn(x, pt, bias=b, out_dtype=out_dtype), (out_dtype, "split 1"))
            for split in (2, 3):
                total = None
                for s in range(split):
                    k0, k1 = 64 * (s * steps // split), min(k, 64 * ((s + 1) * steps // split))
                    ps = packed.pack(p[:, k0:k1].contiguous(), uniform_map((n, k1 - k0), 0), backend="hip")
                    part = packed.linear_wide(x[:, k0:k1].contiguous(), ps).cpu().numpy()
                    with np.errstate(invalid="ignore"):      # Inf - Inf of the specials
                        total = part if total is None else total + part
                if b is not None:
                    total = total + b.cpu().numpy()
                assert total.dtype == np.float32
                got = fn(x, pt, bias=b, out_dtype=out_dtype, split=split)
                _same(got, torch.from_numpy(total).to(dtype).cuda(), (kn, out_dtype, b is not None, split))
                _same(fn(x, pt, bias=b, out_dtype=out_dtype, split=split), got, (kn, out_dtype, split, "again"))


@pytest.mark.parametrize("kn", (False, True))
def test_buffers_stay_whole_and_the_modules_take_the_split(kn):
    m, n, k = 40, 70, 2100
    x, bias, pt, _p = _inexact(m, n, k, kn)
    fn, call, size, mod = (packed.matmul_wide, hb.packed_matmul_wide_split, hb.packed_matmul_wide_split_workspace, packed.PackedMatmul) if kn else \
        (packed.linear_wide, hb.packed_linear_wide_split, hb.packed_linear_wide_split_workspace, packed.PackedLinear)
    assert hb.packed_wide_split(m, n, k, 0) > 1
    for split in (0, 3):
        need = size(m, n, k, split)
        assert need == (hb.packed_wide_split(m, n, k, split) * m * n * 4 + 15) // 16 * 16
        for out_dtype, dtype in DTYPES:
            buf = torch.full((m + 2, n + 5), -7.0, dtype=dtype, device="cuda")
            ws = torch.full((need + 16 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[1:1 + m, 2:2 + n]
            got = call(x, pt.data, pt.tables(), n, bias=bias, out_dtype=dtype, out=out, split=split, workspace=ws[:need + 16])
            assert got.data_ptr() == out.data_ptr()
            _same(out, fn(x, pt, bias=bias, out_dtype=out_dtype, split=split), (kn, split, out_dtype))
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[1:1 + m, 2:2 + n] = False
            assert bool((buf[outside] == -7.0).all()) and bool((ws[need:] == 0xA5).all())
    for out_dtype, _dtype in DTYPES:
        layer = mod(pt, bias=bias, out_dtype=out_dtype, wide_split=0)
        want = fn(x, pt, bias=bias, out_dtype=out_dtype, split=0)
        for _ in range(2):                                  # the second call reuses the kept workspace
            _same(layer(x.reshape(2, m // 2, k)).reshape(m, n), want, (kn, out_dtype, "module"))
        assert layer._wide_workspace.numel() == size(m, n, k, 0)
