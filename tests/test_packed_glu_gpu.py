"""GPU: the gated product on packed weights — packed_glu_wide_kernel and packed_glu_wide_grouped_kernel (WT = false) and glu_combine_kernel of
csrc/mtq_packed.hip, the one activation function of csrc/mtq_glu.hpp — and what packed.py builds on them.

The fused block is 128 (M) × 64 (hidden N) × 64 (K): four waves, each staging one of four tile-row slots that alternate between the gate
and the up stream.  The shapes are the smallest at which that block can go wrong:

  m = 1, 33, 257, 300   the wide tests' rows: one row, a second 32-row MFMA block of one row, a third row block of one row, and three
                        row blocks ragged inside an MFMA block;
  n = 40                one column block whose second tile row is ragged (8 of 32): slots 2 and 3 hold it from both streams;
  n = 72                a second column block whose first tile row is ragged (8 of 32) and whose second is absent (slots 2, 3 without tiles);
  n = 200               four column blocks, the last with a ragged (8 of 32) and an absent tile row;
  k = 100, 300          the element-wise X path, two and five steps, the last tile column ragged;
  k = 104, 320          a contiguous X with k % 8 == 0: the 16-byte X path, ragged and whole;
  (300, 200, 2100)      33 steps, once.

Maps: the gate's random over all four codes, the up's random from another seed (neighbouring waves decode different formats), and both
all-bfp4.

  * bit contract: glu(kernel="fused") == glu(kernel="unfused") — two block-kernel calls into float32 and mtq_glu_combine — on the
    words: both acts, both output types, the four bias combinations, X contiguous and at an unaligned pitch, Y into a pitched buffer
    whose sentinels stay, every call twice; heavy-tailed weights and, NaN-aware, the specials tensor; exchanging gate and up changes
    the heavy result (a test that could not see the streams exchanged would pass nothing);
  * exact arithmetic, independent of the block kernel: act="none" on the integer grid (tests/packed_cases.py, the weights and biases
    coarsened to 2⁻⁴ so that every g·u is a float32: asserted on the CPU) EQUALS the float64 emulation;
  * accuracy of silu against the float64 emulation within the bound stated at _silu_bound, its constant from the sweep below;
  * the sweep: glu_combine at u = 1 over every 2¹⁰-th float32 bit pattern of [−100, 100] against float64: the measured maximum is what
    DESIGN.md §A.6o records (packed.GLU_SILU_MAX_ULPS), and below the point where expf(−g) overflows the result is −0;
  * guards over buffers that stay whole: the gate's packed_bytes cut short of its last tile, map codes 4 and −1 in the up's map: zeros
    for that tile in its own projection only, and the unfused route's bits under the same damage;
  * glu_combine alone, pitched operands and sentinels;
  * grouped: five experts (three for the routing that meets the slot bound) under the grouped wide tests' routings: fused == unfused,
    == glu(kernel="unfused") per expert, rows of no group keep what `out` held, a decreasing group_rows is clamped, a blob past its own
    group's range in the up arena reads as zeros in that expert's up projection only;
  * PackedMLP and PackedExpertsMLP equal their written-out compositions; m = 0 is empty.
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
from tests.test_packed_grouped_gpu import _case, _covered, _rows_dev

pytestmark = pytest.mark.gpu
SHAPES = [(m, n, k) for m in (1, 33, 257, 300) for n in (40, 72, 200) for k in (100, 300)] + [(300, 200, 2100)]
SHAPES += [(1, 72, 320), (33, 200, 104), (257, 40, 104), (300, 200, 320)]       # k % 8 == 0: the 16-byte loads of X
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
ACTS = ("silu", "none")
GLU_GRID = 2.0 ** -4                                     # the grid of the exact tests' weights and biases: see _coarse_grid
U24 = 2.0 ** -24
FLOOR = 2.0 ** -126
SILU_SLOPE_MAX = packed.GLU_SILU_SLOPE_MAX               # 1.1: tests/test_packed_glu_host.py holds max |silu'| below it
# c of the bound: twice the measured error of glu_value's silu plus 2 for the product's rounding and the output's
C = 2.0 * packed.GLU_SILU_MAX_ULPS + 2.0
# expf(-g) is finite up to here: float32's largest finite value is e^88.7228...; the sweep's constant is measured on g >= -SILU_RANGE
SILU_RANGE = 88.72


def _what(w: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """Ŵ as float64, from the oracle."""
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _x_dev(x: np.ndarray):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).cuda()


def _bits(t) -> np.ndarray:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _maps(n, k):
    """(name, the gate's map, the up's map)"""
    return (("random", random_map((n, k), n + k), random_map((n, k), n + k + 1000)), ("bfp4", uniform_map((n, k), 2), uniform_map((n, k), 2)))


@functools.lru_cache(maxsize=None)
def _weights(n, k, kind, which):
    """(packed gate, packed up, gate bias, up bias) of (n, k) on the device — made once per (n, k, values, maps), never written to."""
    if kind == "specials":
        wg, wu = specials((n, k), seed=n + k), specials((n, k), seed=n + k + 5)
    else:
        wg, wu = gen("heavy_f32", 7 * n + k, (n, k)), gen("heavy_f32", 7 * n + k + 5, (n, k))
    _name, mg, mu = next(v for v in _maps(n, k) if v[0] == which)
    if which == "random":
        assert not np.array_equal(mg, mu)
    return (packed.pack(wg, mg, backend="hip"), packed.pack(wu, mu, backend="hip"),
            torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda(), torch.from_numpy(gen("normal_f32", n + 3 * k + 1, (n,))).cuda())


@functools.lru_cache(maxsize=None)
def _x(m, k):
    x = _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 40))
    pitched = torch.zeros((m, k + 9), dtype=torch.bfloat16, device="cuda")
    pitched[:, 1:1 + k] = x
    view = pitched[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and (m == 1 or view.stride(0) % 8 != 0)   # the scalar load path
    return x, view


def _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype):
    """hb.packed_glu_wide into a pitched view of a buffer of sentinels → the (m, n) result; the columns and rows around it stay."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_glu_wide(xd, gate.data, gate.tables(), up.data, up.tables(), n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype, out=out)
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
    for which, _mg, _mu in _maps(n, k):
        gate, up, bgd, bud = _weights(n, k, kind, which)
        for layout, xd in (("contiguous", plain), ("pitched", pitched)):
            for act in ACTS:
                for out_dtype, dtype in DTYPES:
                    for bg, bu in ((None, None), (bgd, None), (None, bud), (bgd, bud)):
                        what = (m, n, k, kind, which, layout, act, out_dtype, bg is not None, bu is not None)
                        unfused = packed.glu(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="unfused")
                        assert tuple(unfused.shape) == (m, n) and unfused.dtype == dtype
                        y = packed.glu(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="fused")
                        assert tuple(y.shape) == (m, n) and y.dtype == dtype
                        _same(y, unfused, kind == "specials", what)
                        first = _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype)
                        _same(first, unfused, kind == "specials", what)
                        again = _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype)
                        assert np.array_equal(_bits(again), _bits(first)), what
        if kind == "heavy":                              # the streams are told apart: exchanged, the result changes
            for act in ACTS:
                there = packed.glu(plain, gate, up, act=act, bias_gate=bgd, kernel="fused")
                back = packed.glu(plain, up, gate, act=act, bias_gate=bgd, kernel="fused")
                assert not np.array_equal(_bits(there), _bits(back)), (m, n, k, which, act)
                _same(back, packed.glu(plain, up, gate, act=act, bias_gate=bgd, kernel="unfused"), False, (m, n, k, which, act, "exchanged"))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_fused_is_the_unfused_route_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy")


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_fused_is_the_unfused_route_on_specials(m, n, k):
    _bit_contract(m, n, k, "specials")
    gate, up, _bg, _bu = _weights(n, k, "specials", "random")
    y = packed.glu(_x(m, k)[0], gate, up, kernel="fused")
    assert m * n < 200 or not bool(torch.isfinite(y).all())                  # the specials reach the output


# ----------------------------------------------------------------------------- exact arithmetic, independent of the block kernel

def _coarse_grid(a: np.ndarray) -> np.ndarray:
    """The integer-grid construction's weights and biases (2⁻⁸, |w| < 1) rounded to 2⁻⁴: g and u are then multiples of 2⁻⁴ below 2⁸ at
    these shapes, and their product, a multiple of 2⁻⁸ below 2¹⁶, is a float32.  At 2⁻⁸ it is not: 30 bits.  The assertion that it is
    stands in the test, for the seeds used."""
    return (np.round(a / GLU_GRID) * GLU_GRID).astype(np.float32)


def _grid_pair(m, n, k, seed):
    x, wg, bg = _grid_case(m, n, k, seed)
    _x_, wu, bu = _grid_case(m, n, k, seed + 1)
    return x, _coarse_grid(wg), _coarse_grid(bg), _coarse_grid(wu), _coarse_grid(bu)


def _exact_product(x, what_g, bg, what_u, bu):
    """g64 * u64 on the grid, asserted to be a float32 (and so its own rounding)."""
    for what, b in ((what_g, bg), (what_u, bu)):
        _grid_preconditions(x, what, b.astype(np.float64))
    x64 = x.astype(np.float64)
    g64, u64 = x64 @ what_g.T + bg.astype(np.float64)[None, :], x64 @ what_u.T + bu.astype(np.float64)[None, :]
    want = g64 * u64
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(want).max() > 1.0
    return want


@pytest.mark.parametrize("m,n,k", [(300, 200, 300), (257, 72, 2100), (300, 200, 320), (33, 40, 104)])
def test_act_none_on_the_integer_grid_equals_the_float64_product(m, n, k):
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 1000 * m + 10 * n + k)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda()
    zero = np.zeros(n, dtype=np.float32)
    for which, mg, mu in _maps(n, k):
        what_g, what_u = _what(wg, mg), _what(wu, mu)
        gate, up = packed.pack(wg, mg, backend="hip"), packed.pack(wu, mu, backend="hip")
        for b_g, b_u, d_g, d_u in ((bg, bu, bgd, bud), (zero, bu, None, bud), (bg, zero, bgd, None), (zero, zero, None, None)):
            want = _exact_product(x, what_g, b_g, what_u, b_u)
            emu = packed.glu(x, gate, up, act="none", bias_gate=None if d_g is None else b_g, bias_up=None if d_u is None else b_u, backend="emulation")
            assert np.array_equal(emu.astype(np.float64), want)
            for kernel in ("fused", "unfused"):
                got = packed.glu(xd, gate, up, act="none", bias_gate=d_g, bias_up=d_u, kernel=kernel).cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, which, kernel, np.argwhere(got != want)[:4])
        half = packed.glu(xd, gate, up, act="none", bias_gate=bgd, bias_up=bud, out_dtype="bfloat16", kernel="fused")
        want = _exact_product(x, what_g, bg, what_u, bu)
        assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))), (m, n, k, which)


# ----------------------------------------------------------------------------- accuracy of silu

def _silu64(g):
    return g / (1.0 + np.exp(-g))


def _silu_bound(x, what_g, bg, what_u, bu):
    """(h64, the bound on |h - h64| for a float32 h).

    E_g, E_u: the project's linear bound (k + 2)·2⁻²⁴·(Σ|x||ŵ| + |b|) on the two f32 projections.  With g = g64 + dg,
    u = u64 + du, |dg| <= E_g, |du| <= E_u: silu(g) u - silu(g64) u64 = (silu(g) - silu(g64)) u + silu(g64) du, and |silu'| < 1.1
    everywhere, so the exact activation of the computed projections is within 1.1·E_g·(|u64| + E_u) + |silu(g64)|·E_u of h64.  The
    computed activation adds c·2⁻²⁴·|h64| + 2⁻¹²⁶, c = 2·(glu_value's measured error in units of 2⁻²⁴ relative) + 2 (the product's
    rounding and the output's).  That constant was measured for g >= -SILU_RANGE, below which expf(-g) overflows: every g the kernel can
    have seen, g64 ± E_g, is asserted to lie inside."""
    k = x.shape[1]
    ax, x64 = np.abs(x).astype(np.float64), x.astype(np.float64)
    g64, u64 = x64 @ what_g.T + bg[None, :], x64 @ what_u.T + bu[None, :]
    e_g = (k + 2) * U24 * (ax @ np.abs(what_g).T + np.abs(bg)[None, :])
    e_u = (k + 2) * U24 * (ax @ np.abs(what_u).T + np.abs(bu)[None, :])
    assert (np.abs(g64) + e_g).max() < SILU_RANGE
    h64 = _silu64(g64) * u64
    return h64, SILU_SLOPE_MAX * e_g * (np.abs(u64) + e_u) + np.abs(_silu64(g64)) * e_u + C * U24 * np.abs(h64) + FLOOR


@pytest.mark.parametrize("m,n,k", [(300, 200, 300), (257, 72, 2100), (33, 40, 104), (1, 72, 100)])
def test_silu_is_within_the_stated_bound_of_the_float64_emulation(m, n, k):
    xd, _pitched = _x(m, k)
    x = xd.float().cpu().numpy()
    for which, mg, mu in _maps(n, k):
        gate, up, bgd, bud = _weights(n, k, "heavy", which)
        what_g, what_u = packed.unpack(gate, backend="hip").cpu().numpy().astype(np.float64), packed.unpack(up, backend="hip").cpu().numpy().astype(np.float64)
        assert np.array_equal(what_g, _what(gen("heavy_f32", 7 * n + k, (n, k)), mg))            # the oracle's Ŵ
        for with_bias in (False, True):
            bg = bgd.cpu().numpy().astype(np.float64) if with_bias else np.zeros(n)
            bu = bud.cpu().numpy().astype(np.float64) if with_bias else np.zeros(n)
            h64, bound = _silu_bound(x, what_g, bg, what_u, bu)
            emu = packed.glu_emulation_f64(x, gate, up, "silu", bg if with_bias else None, bu if with_bias else None)
            assert np.allclose(emu, h64, rtol=1e-12, atol=0.0)
            for kernel in ("fused", "unfused"):
                got = packed.glu(xd, gate, up, act="silu", bias_gate=bgd if with_bias else None, bias_up=bud if with_bias else None, kernel=kernel)
                err = np.abs(got.cpu().numpy().astype(np.float64) - h64)
                worst = float((err / bound).max())
                print(f"silu bound: {(m, n, k)} {which} bias={with_bias} {kernel}: max err / bound = {worst:.4f}, max |h64| = {np.abs(h64).max():.4g}")
                assert worst <= 1.0, (m, n, k, which, with_bias, kernel, np.argwhere(err > bound)[:4])


def _sweep_inputs():
    """Every 2¹⁰-th float32 bit pattern of [0, 100] and of [-100, -0]: 0x42C80000 is 100.0."""
    top = 0x42C80000
    pos = np.arange(0, top + 1, 1 << 10, dtype=np.int64).astype(np.uint32)
    g = np.concatenate([(pos | np.uint32(0x80000000))[::-1], pos]).view(np.float32)
    assert g[0] == -100.0 and g[-1] == 100.0 and g.size == 2 * (top // 1024 + 1) and np.all(np.diff(g.astype(np.float64)) >= 0)
    return g


def _relative_ulps(y: np.ndarray, h64: np.ndarray) -> np.ndarray:
    """|y - h64| less the bound's floor 2⁻¹²⁶, in units of 2⁻²⁴·|h64|: the measure the bound's c multiplies."""
    err = np.maximum(np.abs(y.astype(np.float64) - h64) - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err > 0, err / (U24 * np.abs(h64)), 0.0)


def test_the_sweep_of_glu_value_measures_what_the_design_records():
    """mtq_glu_combine at u = 1 against float64 over the sweep.  Asserts only what was measured and recorded, the
    constant in one place, packed.GLU_SILU_MAX_ULPS: the maximum where expf(-g) is finite (g >= -88.7228), rounded up to a hundredth, IS
    that constant; below, where expf(-g) = inf, the sequence gives -0 for a silu of magnitude up to 88.72·e^-88.72 = 2.6e-37 (all of the value is lost
    there, which no constant describes: it is recorded as it is)."""
    g = _sweep_inputs()
    gd = torch.from_numpy(g.reshape(1, -1).copy()).cuda()
    y = hb.glu_combine(gd, torch.ones_like(gd), act="silu").cpu().numpy().reshape(-1)
    assert y.dtype == np.float32 and y.shape == g.shape
    g64 = g.astype(np.float64)
    with np.errstate(over="ignore"):
        s64 = _silu64(g64)
        inside = np.exp(-g64) <= float(np.finfo(np.float32).max)             # where expf(-g) is finite
    assert np.all(g64[~inside] < -SILU_RANGE) and g64[inside].min() < -SILU_RANGE + 0.01
    ulps = _relative_ulps(y, s64)
    worst = float(ulps[inside].max())
    at = g[inside][int(np.argmax(ulps[inside]))]
    print(f"glu_value sweep: {g.size} inputs; expf(-g) finite: max {worst:.4f} units of 2^-24 relative at g = {at!r}; "
          f"below: {int((~inside).sum())} inputs, outputs all -0: {bool(np.all(y[~inside] == 0.0))}, max |silu| there {np.abs(s64[~inside]).max():.3e}")
    assert np.ceil(worst * 100.0) / 100.0 == packed.GLU_SILU_MAX_ULPS, worst
    assert np.all(y[~inside] == 0.0) and np.all(np.signbit(y[~inside])) and np.abs(s64[~inside]).max() < 2.7e-37
    assert np.all(np.isfinite(y))


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
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 77)
    mg, mu = random_map((n, k), 78), random_map((n, k), 79)
    return n, x, packed.pack(wg, mg, backend="hip"), _what(wg, mg), bg, packed.pack(wu, mu, backend="hip"), _what(wu, mu), bu


def _guarded(gate_tables, up_tables, gone_gate, gone_up):
    """Through the given tables: the unfused route's bits under the same damage, and (act none, float32) the exact product with the tiles
    `gone_*` as zeros in their own projection only.  The streams are whole: a kernel without the guard reads real bytes and fails."""
    n, x, gate, what_g, bg, up, what_u, bu = _guard_case()
    for pt in (gate, up):
        assert pt.data.numel() == pt.nbytes == pt.tables().nbytes            # never a shorter buffer
    left_g, left_u = _zeroed(what_g, gate.map.shape[1], gone_gate), _zeroed(what_u, up.map.shape[1], gone_up)
    assert (np.count_nonzero(left_g != what_g) > 0) == bool(gone_gate) and (np.count_nonzero(left_u != what_u) > 0) == bool(gone_up)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg.copy()).cuda(), torch.from_numpy(bu.copy()).cuda()
    want = _exact_product(x, left_g, bg, left_u, bu)
    assert not np.array_equal(want, _exact_product(x, what_g, bg, what_u, bu))
    for act in ACTS:
        for dtype in (torch.float32, torch.bfloat16):
            g = hb.packed_linear(xd, gate.data, gate_tables, n, bias=bgd, out_dtype=torch.float32)
            u = hb.packed_linear(xd, up.data, up_tables, n, bias=bud, out_dtype=torch.float32)
            unfused = hb.glu_combine(g, u, act=act, out_dtype=dtype)
            y = hb.packed_glu_wide(xd, gate.data, gate_tables, up.data, up_tables, n, act=act, bias_gate=bgd, bias_up=bud, out_dtype=dtype)
            assert np.array_equal(_bits(y), _bits(unfused)), (act, dtype)
            if act == "none" and dtype == torch.float32:
                got = y.cpu().numpy().astype(np.float64)
                assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_a_gate_blob_past_its_packed_bytes_reads_as_zeros_in_the_gate_only():
    _n, _x_, gate, _wg, _bg, up, _wu, _bu = _guard_case()
    last = gate.map.size - 1
    cut = int(gate.offsets[last]) * 64 + TILE_BYTES[int(gate.map.reshape(-1)[last])] - 64      # 64 bytes short of the end of the last tile
    assert gate.map.size * TILE_BYTES[3] <= cut < gate.nbytes                # the entries refuse less
    short = copy.copy(gate.tables())                                         # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    _guarded(short, up.tables(), (last,), ())
    assert gate.tables().nbytes == gate.nbytes                               # the shared tables were not touched


def test_up_tiles_whose_map_code_is_no_format_read_as_zeros_in_the_up_only():
    _n, _x_, gate, _wg, _bg, up, _wu, _bu = _guard_case()
    tiles_h, tiles_w = up.map.shape
    tables = hb.PackedTables.on_device(up.map, up.offsets)                   # a private copy
    inner = (1 * tiles_w + 3, 5 * tiles_w + 6)                               # first column block, second K step; third column block, fourth K step
    assert all(0 < t // tiles_w < tiles_h - 1 and 0 < t % tiles_w < tiles_w - 1 for t in inner)
    tables.map_dev[inner[0]] = 4
    tables.map_dev[inner[1]] = -1
    _guarded(gate.tables(), tables, (), inner)
    assert np.array_equal(up.tables().map_dev.cpu().numpy(), up.map.reshape(-1))


# ----------------------------------------------------------------------------- glu_combine alone

def test_glu_combine_alone_on_pitched_operands():
    rows, cols = 37, 70
    rng = np.random.default_rng(31)
    g = (rng.standard_normal((rows, cols)) * 6).astype(np.float32)
    u = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
    g[0, :4] = [0.0, -0.0, 80.0, -80.0]
    assert np.abs(g).max() < SILU_RANGE
    gbuf = torch.full((rows + 1, cols + 3), 5.0, dtype=torch.float32, device="cuda")
    ubuf = torch.full((rows + 1, cols + 7), 5.0, dtype=torch.float32, device="cuda")
    gbuf[:rows, 1:1 + cols], ubuf[:rows, 2:2 + cols] = torch.from_numpy(g).cuda(), torch.from_numpy(u).cuda()
    gd, ud = gbuf[:rows, 1:1 + cols], ubuf[:rows, 2:2 + cols]
    h64 = {"silu": (torch.nn.functional.silu(torch.from_numpy(g).double()) * torch.from_numpy(u).double()).numpy(),
           "none": g.astype(np.float64) * u.astype(np.float64)}
    for act in ACTS:
        kept = None
        for _name, dtype in DTYPES:
            ybuf = torch.full((rows + 2, cols + 5), -7.0, dtype=dtype, device="cuda")
            out = ybuf[1:1 + rows, 2:2 + cols]
            assert hb.glu_combine(gd, ud, act=act, out_dtype=dtype, out=out).data_ptr() == out.data_ptr()
            whole = ybuf.float().cpu().numpy()
            inside = np.zeros(whole.shape, dtype=bool)
            inside[1:1 + rows, 2:2 + cols] = True
            assert np.all(whole[~inside] == -7.0)
            assert np.array_equal(_bits(hb.glu_combine(gd.contiguous(), ud.contiguous(), act=act, out_dtype=dtype)), _bits(out)), (act, dtype)
            if dtype == torch.float32:
                kept = out.contiguous()
                got = kept.cpu().numpy()
                if act == "none":
                    assert np.array_equal(got, h64[act].astype(np.float32))  # one rounding
                else:
                    assert np.all(np.abs(got.astype(np.float64) - h64[act]) <= C * U24 * np.abs(h64[act]) + FLOOR)
            else:                                        # the float32 value rounded to nearest even once
                assert np.array_equal(_bits(out), _bits(kept.to(torch.bfloat16))), act
    assert bool((gbuf[rows:] == 5.0).all()) and bool((ubuf[rows:] == 5.0).all())
    empty = hb.glu_combine(gd[:0], ud[:0])
    assert tuple(empty.shape) == (0, cols) and empty.dtype == torch.float32


# ----------------------------------------------------------------------------- grouped

ROUTINGS = {"surplus": (0, 3, 3, 131, 132, 390), "hot": (0, 0, 300, 300, 300, 300), "exact-bound": (0, 129, 258, 387), "one-row": (0, 0, 0, 1, 1, 1)}
GROUPED_CASES = [(r, n, k) for r in ROUTINGS for n, k in ((72, 300), (200, 128))]
SENTINEL = 0xA5


def _grouped_case(count, n, k, total_rows):
    """(gate experts, up experts, x, gate bias, up bias): two arenas of other weights and maps, one X."""
    gates, x, bg = _case(count, n, k, total_rows, 3000 + 7 * n + k)
    ups, _x_, bu = _case(count, n, k, total_rows, 4000 + 7 * n + k)
    return gates, ups, x, bg, bu


def _workspace(total_rows, count, n, k):
    need = hb.packed_glu_wide_grouped_workspace_bytes(total_rows, count, n, k)
    buf = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[:need] = 0xFF
    return buf[:need], buf


def _tables(pts, bases_dev=None, maps_dev=None):
    b = packed.batch_of(pts)
    return b.arena, b.maps_dev if maps_dev is None else maps_dev, b.offsets_dev, b.bases_dev if bases_dev is None else bases_dev


@pytest.mark.parametrize("routing,n,k", GROUPED_CASES)
def test_grouped_fused_is_unfused_and_the_dense_route_per_expert(routing, n, k):
    rows = ROUTINGS[routing]
    count, total_rows = len(rows) - 1, rows[-1]
    gates, ups, x, bgd, bud = _grouped_case(count, n, k, total_rows)
    covered = _covered(rows, total_rows)
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            for bg, bu in ((None, None), (bgd, None), (None, bud), (bgd, bud)):
                what = (routing, n, k, act, out_dtype, bg is not None, bu is not None)
                unfused = packed.glu_grouped(x, list(rows), gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="unfused")
                ws, buf = _workspace(total_rows, count, n, k)
                for r in (list(rows), _rows_dev(rows)):      # the second call over what the first left in the workspace
                    y = packed.glu_grouped(x, r, gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="fused", workspace=ws)
                    assert tuple(y.shape) == (total_rows, n) and y.dtype == dtype
                    assert np.array_equal(_bits(y)[covered], _bits(unfused)[covered]), what
                    assert not bool(y[torch.from_numpy(~covered).cuda()].any())
                    assert bool((buf[-256:] == SENTINEL).all())
                for e in range(count):
                    r0, r1 = rows[e], rows[e + 1]
                    if r1 > r0:
                        dense = packed.glu(x[r0:r1], gates[e], ups[e], act=act, bias_gate=None if bg is None else bg[e],
                                           bias_up=None if bu is None else bu[e], out_dtype=out_dtype, kernel="unfused")
                        assert np.array_equal(_bits(y[r0:r1]), _bits(dense)), (what, e)


def test_grouped_rows_of_no_group_keep_what_out_held_and_bad_rows_are_clamped():
    n, k, total_rows = 72, 300, 200
    gates, ups, x, bgd, bud = _grouped_case(3, n, k, total_rows)
    # (group_rows, the clamped ranges the kernel makes of them)
    cases = (((5, 40, 40, 170), [(5, 40), (40, 40), (40, 170)]),
             ((0, 130, 60, 60), [(0, 130), (130, 130), (60, 60)]),           # decreasing
             ((-5, 130, 130, total_rows + 9), [(0, 130), (130, 130), (130, total_rows)]))
    for rows, clamped in cases:
        for e, (r0, r1) in enumerate(clamped):           # the rule, restated
            assert r0 == min(max(rows[e], 0), total_rows) and r1 == min(max(rows[e + 1], r0), total_rows)
        for out_dtype, dtype in DTYPES:
            xbuf = torch.full((total_rows + 16, k), 3.0, dtype=torch.bfloat16, device="cuda")
            xbuf[:total_rows] = x
            ybuf = torch.full((total_rows + 16, n + 4), -7.0, dtype=dtype, device="cuda")
            out = ybuf[:total_rows, 2:2 + n]
            ws, wbuf = _workspace(total_rows, 3, n, k)
            got = hb.packed_glu_wide_grouped(xbuf[:total_rows], _rows_dev(rows), _tables(gates), _tables(ups), 3, n, bias_gate=bgd, bias_up=bud,
                                             out_dtype=dtype, out=out, workspace=ws)
            assert got.data_ptr() == out.data_ptr()
            assert bool((ybuf[total_rows:] == -7.0).all()) and bool((ybuf[:, :2] == -7.0).all()) and bool((ybuf[:, 2 + n:] == -7.0).all())
            assert bool((wbuf[-256:] == SENTINEL).all())
            written = np.zeros(total_rows, dtype=bool)
            for e, (r0, r1) in enumerate(clamped):
                written[r0:r1] = True
                if r1 > r0:
                    dense = packed.glu(x[r0:r1], gates[e], ups[e], bias_gate=bgd[e], bias_up=bud[e], out_dtype=out_dtype, kernel="unfused")
                    assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (rows, e)
            assert bool((out[torch.from_numpy(~written).cuda()] == -7.0).all()), (rows, "a row of no group was written")


def test_grouped_up_blob_past_its_own_groups_range_reads_as_zeros_in_that_up_projection_only():
    count, n, k, rows = 5, 72, 300, (0, 130, 130, 162, 163, 300)
    total_rows = rows[-1]
    rng = np.random.default_rng(4243)
    x = rng.integers(-4, 5, size=(total_rows, k)).astype(np.float32)
    wg, wu = (_coarse_grid(rng.integers(-255, 256, size=(count, n, k)) * 2.0 ** -8) for _ in range(2))
    bg, bu = (_coarse_grid(rng.integers(-255, 256, size=(count, n)) * 2.0 ** -8) for _ in range(2))
    mg = np.stack([random_map((n, k), 140 + i) for i in range(count)])
    mu = np.stack([random_map((n, k), 150 + i) for i in range(count)])
    what_g, what_u = np.stack([_what(wg[i], mg[i]) for i in range(count)]), np.stack([_what(wu[i], mu[i]) for i in range(count)])
    gates = packed.pack_batch(torch.from_numpy(wg).cuda(), mg, backend="hip")
    ups = packed.pack_batch(torch.from_numpy(wu).cuda(), mu, backend="hip")
    e = 2
    bases = packed.batch_of(ups).bases_dev.clone()
    bases[e + 1] -= 1                                    # the up expert's stream ends one unit early: its last tile does not fit
    tiles_h, tiles_w = ups[0].map.shape
    left_u = what_u.copy()
    left_u[e] = _zeroed(what_u[e], tiles_w, [tiles_h * tiles_w - 1])
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda()
    got = hb.packed_glu_wide_grouped(xd, _rows_dev(rows), _tables(gates), _tables(ups, bases_dev=bases), count, n, act="none", bias_gate=bgd,
                                     bias_up=bud).cpu().numpy().astype(np.float64)
    g = hb.packed_linear_wide_grouped(xd, _rows_dev(rows), *_tables(gates), count, n, bias=bgd)
    u = hb.packed_linear_wide_grouped(xd, _rows_dev(rows), *_tables(ups, bases_dev=bases), count, n, bias=bud)
    unfused = hb.glu_combine(g, u, act="none").cpu().numpy().astype(np.float64)
    for i in (0, 1, 2, 4):                               # up expert 3 now starts a unit early: it reads bytes of the arena that mean nothing
        r0, r1 = rows[i], rows[i + 1]
        if r1 == r0:
            continue
        want = _exact_product(x[r0:r1], what_g[i], bg[i], left_u[i], bu[i])
        assert np.array_equal(got[r0:r1], want), (i, np.argwhere(got[r0:r1] != want)[:4])
        assert np.array_equal(unfused[r0:r1], want), i
        if i == e:
            assert not np.array_equal(want, _exact_product(x[r0:r1], what_g[i], bg[i], what_u[i], bu[i]))
    assert np.array_equal(packed.batch_of(ups).bases_dev.cpu().numpy().view(np.uint64), packed.batch_of(ups).bases)


# ----------------------------------------------------------------------------- modules

def test_the_modules_are_their_written_out_compositions():
    n, k, k_out, m = 72, 100, 40, 70
    gate, up, _bg, _bu = _weights(n, k, "heavy", "random")
    down = packed.pack(gen("heavy_f32", 91, (k_out, n)), random_map((k_out, n), 92), backend="hip")
    x = _x_dev(to_bf16_valued(gen("normal_f32", 93, (m, k)) * 40))
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            mlp = packed.PackedMLP(gate, up, down, act=act, out_dtype=out_dtype)
            assert mlp.backend == "hip" and (mlp.in_features, mlp.hidden_features, mlp.out_features) == (k, n, k_out)
            for rows in (m, 7):                          # above and inside the skinny range
                h = packed.glu(x[:rows], gate, up, act=act, out_dtype="bfloat16", kernel="auto")
                want = packed.linear(h, down, out_dtype=out_dtype, kernel="auto")
                y = mlp(x[:rows])
                assert tuple(y.shape) == (rows, k_out) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), (act, out_dtype, rows)
            assert np.array_equal(_bits(mlp(x.reshape(7, 10, k)).reshape(m, k_out)), _bits(mlp(x)))
            empty = mlp(x[:0])
            assert tuple(empty.shape) == (0, k_out) and empty.dtype == dtype and empty.is_cuda
    rows = (0, 3, 3, 131, 132, 390)
    count, total_rows, k = 5, 390, 300
    gates, ups, xg, _bgd, _bud = _grouped_case(count, n, k, total_rows)
    wd = np.stack([gen("heavy_f32", 95 + i, (k_out, n)) for i in range(count)])
    downs = packed.pack_batch(torch.from_numpy(wd).cuda(), np.stack([random_map((k_out, n), 96 + i) for i in range(count)]), backend="hip")
    for out_dtype, dtype in DTYPES:
        experts = packed.PackedExpertsMLP(gates, ups, downs, out_dtype=out_dtype)
        assert experts.backend == "hip" and (experts.count, experts.in_features, experts.hidden_features, experts.out_features) == (count, k, n, k_out)
        h = packed.glu_grouped(xg, list(rows), gates, ups, out_dtype="bfloat16", kernel="fused")
        want = packed.linear_grouped_wide(h, list(rows), downs, out_dtype=out_dtype)
        for r in (list(rows), _rows_dev(rows)):
            y = experts(xg, r)
            assert tuple(y.shape) == (total_rows, k_out) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), out_dtype
        empty = experts(xg[:0], [0] * (count + 1))
        assert tuple(empty.shape) == (0, k_out) and empty.dtype == dtype
    assert tuple(packed.glu(xg[:0], gates[0], ups[0], kernel="fused").shape) == (0, n)
    assert tuple(packed.glu_grouped(xg[:0], [0] * (count + 1), gates, ups).shape) == (0, n)
