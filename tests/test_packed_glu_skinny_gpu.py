"""GPU: the fused gated product for decode — packed_glu_skinny_kernel + glu_skinny_reduce_kernel and their grouped forms in
csrc/mtq_packed.hip — and what packed.py builds on them.

A wave takes one (slice, projection, tile row) unit and does on its own projection's stream what the skinny linear wave does; the
reduce sums each projection's slices, adds its bias and applies glu_value.  The shapes are the smallest at which that can go wrong:

  m = 1, 5, 32          one row, a ragged MFMA block, the whole block;
  n = 32, 40, 96        one tile row; a second, ragged one (2 tile rows x 2 projections = one workgroup at split 1); three tile rows
                        (six units at split 1: a workgroup and a half, and the projection seam inside a workgroup);
  k = 32, 100, 160      one tile; four tiles, the last ragged; five tiles, below the ring of 8;
  k = 288, 2080         ring + 1; 65 tiles, one past the 64-tile hand-out at split 1 (n = 32 only);
  split = 0, 1, 2, 3, 1000   the library's rule, no split, two and three (uneven) slices, more slices than tile columns.

  * bit contract: y == mtq_packed_linear_skinny on the gate stream with bias_gate into float32 at the same split, the same on the up
    stream, mtq_glu_combine of the two — both acts, both output types, the four bias combinations, random maps over all four codes that
    differ between gate and up, heavy-tailed weights and the specials tensor (and, since under it nearly every output is NaN, the same
    tensor without its Inf / NaN words under rows of X with a single 1.0); at split 0 also == packed.glu(kernel="auto");
  * independent of the pair: act="none" on the integer grid EQUALS the float64 product; silu is within the bound that
    tests/test_packed_glu_gpu.py states against the float64 emulation;
  * guards over buffers that stay whole: the gate's packed_bytes cut short, a map code 7 in the up's map: zeros for that tile in its
    own projection only; y a pitched view of sentinels with spare rows; the workspace exactly the size function's bytes inside
    sentinels; x a pitched, unaligned view;
  * two calls over one workspace give equal bits;
  * grouped: three experts under routings with an empty group, a 70-row group (three chunks), rows of no group at both ends and
    decreasing arrays: == two linear_grouped(kernel="walk") calls and glu_combine, == the dense glu_skinny per group and chunk at the
    effective split, rows of no group keep `out`'s sentinel, a blob past its own group's range reads as zeros in its own projection;
  * PackedMLP(decode_kernel="fused") and PackedExpertsMLP(decode_max_rows=...) against the default module and the compositions.
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
from tests.packed_cases import TILE_BYTES, random_map, specials
from tests.test_packed_glu_gpu import _bits, _coarse_grid, _exact_product, _grid_pair, _silu_bound, _what, _x_dev, _zeroed
from tests.test_packed_grouped_gpu import _case, _rows_dev

pytestmark = pytest.mark.gpu
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
ACTS = ("silu", "none")
SPLITS = (0, 1, 2, 3, 1000)
MS, NS, KS = (1, 5, 32), (32, 40, 96), (32, 100, 160, 288)
LONG_K = 2080
SENTINEL = 0xA5


def _eff(m, n, k, split):
    """The effective split, from the workspace the library asks for: 2 · split_eff · m · n floats rounded up to 16 bytes."""
    need = hb.packed_glu_skinny_workspace_bytes(m, n, k, split)
    assert need >= 2 * 4 * m * n and (m * n * 8 < 16 or need % (8 * m * n) < 16)
    return max(1, need // (8 * m * n))


@functools.lru_cache(maxsize=None)
def _weights(n, k, kind):
    """(packed gate, packed up, gate bias, up bias) of (n, k) on the device — made once, never written to."""
    if kind in ("specials", "finite-specials"):
        wg, wu = specials((n, k), seed=n + k), specials((n, k), seed=n + k + 5)
        if kind == "finite-specials":                    # exponent fields 254 and 255 → 126 and 127: no Inf, no NaN, none by rounding to bf16
            for w in (wg, wu):
                bits = w.view(np.uint32)
                bits[(bits & 0x7F800000) >= 0x7F000000] &= np.uint32(0xBFFFFFFF)
    else:
        wg, wu = gen("heavy_f32", 7 * n + k, (n, k)), gen("heavy_f32", 7 * n + k + 5, (n, k))
    mg, mu = random_map((n, k), n + k), random_map((n, k), n + k + 1000)
    if mg.size >= 4:                                     # every code in both maps, in another order
        mg.reshape(-1)[:4], mu.reshape(-1)[:4] = [0, 1, 2, 3], [3, 2, 1, 0]
    assert mg.size == 1 or not np.array_equal(mg, mu)
    return (packed.pack(wg, mg, backend="hip"), packed.pack(wu, mu, backend="hip"),
            torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda(), torch.from_numpy(gen("normal_f32", n + 3 * k + 1, (n,))).cuda())


@functools.lru_cache(maxsize=None)
def _x(m, k):
    return _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 8))


def _pair(xd, gate, up, n, bg, bu, split):
    """Steps (1) and (2) of the contract: the two skinny calls into float32 at `split`."""
    g = hb.packed_linear_skinny(xd, gate.data, gate.tables(), n, bias=bg, out_dtype=torch.float32, split=split)
    u = hb.packed_linear_skinny(xd, up.data, up.tables(), n, bias=bu, out_dtype=torch.float32, split=split)
    return g, u


def _fused(xd, gate, up, n, act, bg, bu, dtype, split, **kw):
    return hb.packed_glu_skinny(xd, gate.data, gate.tables(), up.data, up.tables(), n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype,
                                split=split, **kw)


def _pair_combine(xd, gate, up, n, act, bg, bu, dtype, split):
    """The contract's right-hand side: the three-step sequence at `split`."""
    g, u = _pair(xd, gate, up, n, bg, bu, split)
    return hb.glu_combine(g, u, act=act, out_dtype=dtype)


def _bit_contract(m, n, k, kind, xd=None):
    xd = _x(m, k) if xd is None else xd
    gate, up, bgd, bud = _weights(n, k, kind)
    tiles_w = (k + 31) // 32
    for split in SPLITS:
        eff = _eff(m, n, k, split)
        assert eff == min(tiles_w, split) if split else eff == max(1, min(2048 // ((n + 31) // 32), tiles_w // 4))
        sides = {(has_g, has_u): _pair(xd, gate, up, n, bgd if has_g else None, bud if has_u else None, split)
                 for has_g in (False, True) for has_u in (False, True)}
        for (has_g, has_u), (g, u) in sides.items():
            bg, bu = bgd if has_g else None, bud if has_u else None
            for act in ACTS:
                for out_dtype, dtype in DTYPES:
                    what = (m, n, k, kind, split, act, out_dtype, has_g, has_u)
                    want = hb.glu_combine(g, u, act=act, out_dtype=dtype)
                    y = _fused(xd, gate, up, n, act, bg, bu, dtype, split)
                    assert tuple(y.shape) == (m, n) and y.dtype == dtype
                    assert np.array_equal(_bits(y), _bits(want)), (what, np.argwhere(_bits(y) != _bits(want))[:4])
                    if split == 0:
                        auto = packed.glu(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="auto")
                        top = packed.glu_skinny(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype)
                        assert np.array_equal(_bits(auto), _bits(want)) and np.array_equal(_bits(top), _bits(want)), what
    if kind == "heavy" and n * k > 32 * 32:              # the streams are told apart: exchanged, the result changes
        there = _fused(xd, gate, up, n, "silu", bgd, None, torch.float32, 0)
        back = _fused(xd, up, gate, n, "silu", bgd, None, torch.float32, 0)
        assert not np.array_equal(_bits(there), _bits(back)), (m, n, k)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_fused_is_the_skinny_pair_and_the_combine_bit_for_bit(m, n):
    for k in KS:
        _bit_contract(m, n, k, "heavy")


@pytest.mark.parametrize("m", MS)
def test_fused_is_the_pair_over_a_run_longer_than_the_hand_out(m):
    assert (LONG_K + 31) // 32 == 65 and _eff(m, 32, LONG_K, 0) == 16 and _eff(m, 32, LONG_K, 1) == 1
    _bit_contract(m, 32, LONG_K, "heavy")


@pytest.mark.parametrize("m,n,k", [(5, 40, 100), (32, 96, 288), (1, 32, LONG_K), (32, 40, 160)])
def test_fused_is_the_pair_on_specials(m, n, k):
    _bit_contract(m, n, k, "specials")
    gate, up, _bg, _bu = _weights(n, k, "specials")
    y = _fused(_x(m, k), gate, up, n, "silu", None, None, torch.float32, 0)
    assert m * n < 200 or not bool(torch.isfinite(y).all())                  # the specials reach the output
    # A row of the specials holds an Inf or a NaN almost surely, so nearly every output above is NaN, and NaN == NaN tells no stream,
    # map or projection apart.  The same tensor with its Inf / NaN words made finite keeps -0, the denormals and both ends of the exponent
    # range; under rows of X with a single 1.0 (0 · finite = 0) g and u are single decoded words and the bits of most outputs say
    # where they came from.  The columns picked are those with the most outputs whose g · u is a finite normal float32.
    gate, up, _bg, _bu = _weights(n, k, "finite-specials")
    wg, wu = packed.unpack(gate, backend="hip").cpu().numpy(), packed.unpack(up, backend="hip").cpu().numpy()
    assert np.isfinite(wg).all() and np.isfinite(wu).all()
    with np.errstate(over="ignore", under="ignore"):
        prod = wg * wu
    tiny = np.float32(2.0 ** -126)                       # normal operands and a normal product: nothing hangs on how denormals are treated
    good = np.isfinite(prod) & (np.abs(prod) >= tiny) & (np.abs(wg) >= tiny) & (np.abs(wu) >= tiny)
    cols = np.argsort(-good.sum(axis=0), kind="stable")[:m]
    pick = np.zeros((m, k), dtype=np.float32)
    pick[np.arange(m), cols] = 1.0
    xd = _x_dev(pick)
    _bit_contract(m, n, k, "finite-specials", xd=xd)
    _bit_contract(m, n, k, "finite-specials")
    y = _fused(xd, gate, up, n, "none", None, None, torch.float32, 0).cpu().numpy()
    want = prod[:, cols].T                               # one product, one rounding
    assert int(good[:, cols].sum()) >= max(1, m * n // 16), int(good[:, cols].sum())
    assert np.array_equal(y.view(np.uint32)[good[:, cols].T], want.view(np.uint32)[good[:, cols].T])
    back = _fused(xd, up, gate, n, "silu", None, None, torch.float32, 0).cpu().numpy()
    there = _fused(xd, gate, up, n, "silu", None, None, torch.float32, 0).cpu().numpy()
    assert not np.array_equal(there.view(np.uint32), back.view(np.uint32))    # silu(g) · u is not silu(u) · g


# ----------------------------------------------------------------------------- independent of the pair

@pytest.mark.parametrize("m,n,k", [(32, 96, 288), (5, 40, 100), (7, 32, LONG_K)])
def test_act_none_on_the_integer_grid_equals_the_float64_product(m, n, k):
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 1000 * m + 10 * n + k)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda()
    zero = np.zeros(n, dtype=np.float32)
    mg, mu = random_map((n, k), n + k), random_map((n, k), n + k + 1000)
    what_g, what_u = _what(wg, mg), _what(wu, mu)
    gate, up = packed.pack(wg, mg, backend="hip"), packed.pack(wu, mu, backend="hip")
    for b_g, b_u, d_g, d_u in ((bg, bu, bgd, bud), (zero, bu, None, bud), (bg, zero, bgd, None), (zero, zero, None, None)):
        want = _exact_product(x, what_g, b_g, what_u, b_u)
        for split in SPLITS:                             # exact sums: every split gives the same value
            got = _fused(xd, gate, up, n, "none", d_g, d_u, torch.float32, split).cpu().numpy()
            assert got.shape == (m, n) and got.dtype == np.float32
            assert np.array_equal(got.astype(np.float64), want), (m, n, k, split, np.argwhere(got != want)[:4])
    half = _fused(xd, gate, up, n, "none", bgd, bud, torch.bfloat16, 0)
    want = _exact_product(x, what_g, bg, what_u, bu)
    assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))), (m, n, k)


@pytest.mark.parametrize("m,n,k", [(32, 96, 288), (5, 40, 100), (1, 32, LONG_K)])
def test_silu_is_within_the_stated_bound_of_the_float64_emulation(m, n, k):
    """The bound of tests/test_packed_glu_gpu.py's test of the same name (_silu_bound there: GLU_SILU_MAX_ULPS, GLU_SILU_SLOPE_MAX and
    the (k + 2)·2⁻²⁴ linear bound, which holds for any order of the K sum and so for every split)."""
    xd = _x(m, k)
    x = xd.float().cpu().numpy()
    gate, up, bgd, bud = _weights(n, k, "heavy")
    what_g = packed.unpack(gate, backend="hip").cpu().numpy().astype(np.float64)
    what_u = packed.unpack(up, backend="hip").cpu().numpy().astype(np.float64)
    assert np.array_equal(what_g, _what(gen("heavy_f32", 7 * n + k, (n, k)), gate.map))             # the oracle's Ŵ
    for with_bias in (False, True):
        bg = bgd.cpu().numpy().astype(np.float64) if with_bias else np.zeros(n)
        bu = bud.cpu().numpy().astype(np.float64) if with_bias else np.zeros(n)
        h64, bound = _silu_bound(x, what_g, bg, what_u, bu)
        emu = packed.glu_emulation_f64(x, gate, up, "silu", bg if with_bias else None, bu if with_bias else None)
        assert np.allclose(emu, h64, rtol=1e-12, atol=0.0)
        for split in (0, 1, 3):
            got = _fused(xd, gate, up, n, "silu", bgd if with_bias else None, bud if with_bias else None, torch.float32, split)
            err = np.abs(got.cpu().numpy().astype(np.float64) - h64)
            worst = float((err / bound).max())
            print(f"silu bound: {(m, n, k)} bias={with_bias} split={split}: max err / bound = {worst:.4f}, max |h64| = {np.abs(h64).max():.4g}")
            assert worst <= 1.0, (m, n, k, with_bias, split, np.argwhere(err > bound)[:4])


# ----------------------------------------------------------------------------- guards

@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 21, 96, 288
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 77)
    mg, mu = random_map((n, k), 78), random_map((n, k), 79)
    return n, x, packed.pack(wg, mg, backend="hip"), _what(wg, mg), bg, packed.pack(wu, mu, backend="hip"), _what(wu, mu), bu


def _guarded(gate_tables, up_tables, gone_gate, gone_up):
    """Through the given tables: the pair's bits under the same damage, and (act none, float32) the exact product with the tiles `gone_*`
    as zeros in their own projection only.  The streams are whole: a kernel without the guard reads real bytes and fails."""
    n, x, gate, what_g, bg, up, what_u, bu = _guard_case()
    for pt in (gate, up):
        assert pt.data.numel() == pt.nbytes == pt.tables().nbytes            # never a shorter buffer
    left_g, left_u = _zeroed(what_g, gate.map.shape[1], gone_gate), _zeroed(what_u, up.map.shape[1], gone_up)
    assert (np.count_nonzero(left_g != what_g) > 0) == bool(gone_gate) and (np.count_nonzero(left_u != what_u) > 0) == bool(gone_up)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg.copy()).cuda(), torch.from_numpy(bu.copy()).cuda()
    want = _exact_product(x, left_g, bg, left_u, bu)
    assert not np.array_equal(want, _exact_product(x, what_g, bg, what_u, bu))
    for split in (0, 1, 3):
        for act in ACTS:
            for dtype in (torch.float32, torch.bfloat16):
                g = hb.packed_linear_skinny(xd, gate.data, gate_tables, n, bias=bgd, out_dtype=torch.float32, split=split)
                u = hb.packed_linear_skinny(xd, up.data, up_tables, n, bias=bud, out_dtype=torch.float32, split=split)
                pair = hb.glu_combine(g, u, act=act, out_dtype=dtype)
                y = hb.packed_glu_skinny(xd, gate.data, gate_tables, up.data, up_tables, n, act=act, bias_gate=bgd, bias_up=bud, out_dtype=dtype,
                                         split=split)
                assert np.array_equal(_bits(y), _bits(pair)), (split, act, dtype)
                if act == "none" and dtype == torch.float32:
                    got = y.cpu().numpy().astype(np.float64)
                    assert np.array_equal(got, want), (split, np.argwhere(got != want)[:4])


def test_a_gate_blob_past_its_packed_bytes_reads_as_zeros_in_the_gate_only():
    _n, _x_, gate, _wg, _bg, up, _wu, _bu = _guard_case()
    last = gate.map.size - 1
    cut = int(gate.offsets[last]) * 64 + TILE_BYTES[int(gate.map.reshape(-1)[last])] - 64      # 64 bytes short of the end of the last tile
    assert gate.map.size * TILE_BYTES[3] <= cut < gate.nbytes                # the entries refuse less
    short = copy.copy(gate.tables())                                         # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    _guarded(short, up.tables(), (last,), ())
    assert gate.tables().nbytes == gate.nbytes                               # the shared tables were not touched


def test_an_up_tile_with_map_code_7_reads_as_zeros_in_the_up_only():
    _n, _x_, gate, _wg, _bg, up, _wu, _bu = _guard_case()
    tiles_h, tiles_w = up.map.shape
    tables = hb.PackedTables.on_device(up.map, up.offsets)                   # a private copy
    inner = (1 * tiles_w + 3,)                                               # second tile row, fourth K step: slice 1 of 3
    assert (tiles_h, tiles_w) == (3, 9)
    tables.map_dev[inner[0]] = 7
    _guarded(gate.tables(), tables, (), inner)
    assert np.array_equal(up.tables().map_dev.cpu().numpy(), up.map.reshape(-1))


def _workspace(need):
    """(a slice of exactly `need` bytes, the sentinel-filled allocation around it)"""
    buf = torch.full((256 + need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = buf[256:256 + need]
    assert ws.data_ptr() % 16 == 0
    return ws, buf


def _untouched_around(buf, need):
    return bool((buf[:256] == SENTINEL).all()) and bool((buf[256 + need:] == SENTINEL).all())


@pytest.mark.parametrize("m,n,k", [(5, 40, 100), (21, 96, 288), (1, 32, LONG_K)])
def test_nothing_outside_y_or_the_workspace_is_written_and_x_may_be_pitched(m, n, k):
    xd = _x(m, k)
    gate, up, bgd, bud = _weights(n, k, "heavy")
    xbuf = torch.full((m + 3, k + 9), 3.0, dtype=torch.bfloat16, device="cuda")          # rows past m and columns past k hold 3.0
    xbuf[:m, 1:1 + k] = xd
    view = xbuf[:m, 1:1 + k]
    assert view.data_ptr() % 16 != 0                     # the element-wise loads of X
    for split in SPLITS:
        need = hb.packed_glu_skinny_workspace_bytes(m, n, k, split)
        for act in ACTS:
            for _name, dtype in DTYPES:
                want = _pair_combine(xd, gate, up, n, act, bgd, bud, dtype, split)   # on the contiguous x
                ws, wbuf = _workspace(need)
                ybuf = torch.full((m + 4, n + 5), -7.0, dtype=dtype, device="cuda")
                out = ybuf[1:1 + m, 2:2 + n]             # ldy > n, and rows of the buffer after the last
                got = _fused(view, gate, up, n, act, bgd, bud, dtype, split, out=out, workspace=ws)
                assert got.data_ptr() == out.data_ptr()
                whole = ybuf.float().cpu().numpy()
                inside = np.zeros(whole.shape, dtype=bool)
                inside[1:1 + m, 2:2 + n] = True
                assert np.all(whole[~inside] == -7.0), (split, act, dtype, np.argwhere((whole != -7.0) & ~inside)[:4])
                assert _untouched_around(wbuf, need), (split, act, dtype)
                assert np.array_equal(_bits(out), _bits(want)), (split, act, dtype)
                first = _bits(out).copy()                # the second call over what the first left in the workspace
                again = _fused(view, gate, up, n, act, bgd, bud, dtype, split, out=out, workspace=ws)
                assert np.array_equal(_bits(again), first) and _untouched_around(wbuf, need), (split, act, dtype)
    assert bool((xbuf[m:] == 3.0).all())
    with pytest.raises(hb.MtqError, match="workspace"):
        short = hb.packed_glu_skinny_workspace_bytes(m, n, k, 1) - 16        # at split 1 too
        _fused(xd, gate, up, n, "silu", None, None, torch.float32, 1, workspace=torch.empty((short,), dtype=torch.uint8, device="cuda"))
    with pytest.raises(hb.MtqError, match="m <= 32"):
        packed.glu_skinny(torch.zeros((33, k), dtype=torch.bfloat16, device="cuda"), gate, up)
    assert tuple(packed.glu_skinny(xd[:0], gate, up).shape) == (0, n)


def test_two_calls_that_share_a_workspace_on_one_stream_give_equal_bits():
    m, n, k = 32, 96, 288
    xa, xb = _x(m, k), _x_dev(to_bf16_valued(gen("normal_f32", 5, (m, k)) * 8))
    gate, up, bgd, bud = _weights(n, k, "heavy")
    for split in (0, 3):
        ws = torch.empty((hb.packed_glu_skinny_workspace_bytes(m, n, k, split),), dtype=torch.uint8, device="cuda")
        alone_a = _pair_combine(xa, gate, up, n, "silu", bgd, bud, torch.float32, split)
        alone_b = _pair_combine(xb, up, gate, n, "silu", bgd, bud, torch.float32, split)
        outs = []
        for _round in range(3):                          # back to back, no synchronisation between them: the stream orders them
            outs.append((_fused(xa, gate, up, n, "silu", bgd, bud, torch.float32, split, workspace=ws),
                         _fused(xb, up, gate, n, "silu", bgd, bud, torch.float32, split, workspace=ws)))
        for a, b in outs:
            assert np.array_equal(_bits(a), _bits(alone_a)) and np.array_equal(_bits(b), _bits(alone_b)), split
        assert not np.array_equal(_bits(alone_a), _bits(alone_b))


# ----------------------------------------------------------------------------- grouped

COUNT = 3
GROUPED_SHAPES = ((40, 100), (96, 288))
# (group_rows, total_rows): an empty group; one group of 70 rows (three chunks, the last of 6); rows 0..3 and 25..29 of no group
ROUTINGS = {"empty": ((0, 5, 5, 21), 21), "hot": ((0, 0, 70, 70), 70), "uncovered": ((4, 9, 9, 25), 30)}


def _grouped_case(n, k, total_rows):
    gates, x, bg = _case(COUNT, n, k, total_rows, 3000 + 7 * n + k)
    ups, _x_, bu = _case(COUNT, n, k, total_rows, 4000 + 7 * n + k)
    return gates, ups, x, bg, bu


def _tables(pts, bases_dev=None):
    b = packed.batch_of(pts)
    return b.arena, b.maps_dev, b.offsets_dev, b.bases_dev if bases_dev is None else bases_dev


def _eff_grouped(total_rows, n, k, split):
    need = hb.packed_glu_skinny_grouped_workspace_bytes(total_rows, COUNT, n, k, split)
    return max(1, need // (8 * total_rows * n)), need


def _grouped_into_sentinels(x, rows_dev, gates, ups, n, act, bg, bu, dtype, split, total_rows, k):
    eff, need = _eff_grouped(total_rows, n, k, split)
    ws, wbuf = _workspace(need)
    ybuf = torch.full((total_rows + 3, n + 4), -7.0, dtype=dtype, device="cuda")
    out = ybuf[:total_rows, 2:2 + n]
    got = hb.packed_glu_skinny_grouped(x, rows_dev, _tables(gates), _tables(ups), COUNT, n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype,
                                       out=out, split=split, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    assert bool((ybuf[total_rows:] == -7.0).all()) and bool((ybuf[:, :2] == -7.0).all()) and bool((ybuf[:, 2 + n:] == -7.0).all())
    assert _untouched_around(wbuf, need)
    return out, eff


@pytest.mark.parametrize("n,k", GROUPED_SHAPES)
@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_grouped_is_the_two_walks_and_the_combine_and_the_dense_call_per_group(routing, n, k):
    rows, total_rows = ROUTINGS[routing]
    gates, ups, x, bgd, bud = _grouped_case(n, k, total_rows)
    covered = np.zeros(total_rows, dtype=bool)
    for e in range(COUNT):
        covered[rows[e]:rows[e + 1]] = True
    keep = torch.from_numpy(~covered).cuda()
    # the walks take checked host arrays only when the groups cover every row: the kernel's own reading of the array otherwise
    r = _rows_dev(rows)
    for split in (0, 1, 2):
        for with_bias in (False, True):
            bg, bu = (bgd, bud) if with_bias else (None, None)
            g = packed.linear_grouped(x, r, gates, bias=bg, out_dtype="float32", split=split, kernel="walk")
            u = packed.linear_grouped(x, r, ups, bias=bu, out_dtype="float32", split=split, kernel="walk")
            for act in ACTS:
                for out_dtype, dtype in DTYPES:
                    what = (routing, n, k, split, with_bias, act, out_dtype)
                    want = hb.glu_combine(g, u, act=act, out_dtype=dtype)
                    out, eff = _grouped_into_sentinels(x, r, gates, ups, n, act, bg, bu, dtype, split, total_rows, k)
                    assert np.array_equal(_bits(out)[covered], _bits(want)[covered]), what
                    assert bool((out[keep] == -7.0).all()), (what, "a row of no group was written")
                    top = packed.glu_grouped_skinny(x, r, gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, split=split)
                    assert np.array_equal(_bits(top)[covered], _bits(want)[covered]) and not bool(top[keep].any()), what
                    for e in range(COUNT):               # the dense call on every 32-row chunk of every group, at the effective split
                        for r0 in range(rows[e], rows[e + 1], 32):
                            r1 = min(r0 + 32, rows[e + 1])
                            dense = packed.glu_skinny(x[r0:r1], gates[e], ups[e], act=act, bias_gate=None if bg is None else bg[e],
                                                      bias_up=None if bu is None else bu[e], out_dtype=out_dtype, split=eff)
                            assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (what, e, r0)
    if routing == "empty":                               # a checked host array gives the same call
        host = packed.glu_grouped_skinny(x, list(rows), gates, ups, bias_gate=bgd, bias_up=bud)
        assert np.array_equal(_bits(host), _bits(packed.glu_grouped_skinny(x, r, gates, ups, bias_gate=bgd, bias_up=bud)))
        assert tuple(packed.glu_grouped_skinny(x[:0], [0] * (COUNT + 1), gates, ups).shape) == (0, n)


@pytest.mark.parametrize("n,k", GROUPED_SHAPES)
def test_grouped_decreasing_rows_are_clamped_and_stay_in_bounds(n, k):
    total_rows = 30
    gates, ups, x, bgd, bud = _grouped_case(n, k, total_rows)
    # (group_rows, the clamped ranges the kernel makes of them, the groups that overlap no other)
    cases = (((10, 30, 0, 8), [(10, 30), (30, 30), (0, 8)], (0, 2)),
             ((0, 21, 9, 9), [(0, 21), (21, 21), (9, 9)], (0,)),
             ((-5, 12, 12, total_rows + 9), [(0, 12), (12, 12), (12, 30)], (0, 2)),
             ((0, 20, 10, 30), [(0, 20), (20, 20), (10, 30)], ()))           # groups 0 and 2 share rows 10..19: in bounds, nothing more
    for rows, clamped, alone in cases:
        for e, (r0, r1) in enumerate(clamped):           # the rule, restated
            assert r0 == min(max(rows[e], 0), total_rows) and r1 == min(max(rows[e + 1], r0), total_rows)
        for split in (0, 2):
            for out_dtype, dtype in DTYPES:
                xbuf = torch.full((total_rows + 16, k), 3.0, dtype=torch.bfloat16, device="cuda")
                xbuf[:total_rows] = x
                out, eff = _grouped_into_sentinels(xbuf[:total_rows], _rows_dev(rows), gates, ups, n, "silu", bgd, bud, dtype, split, total_rows, k)
                written = np.zeros(total_rows, dtype=bool)
                for e, (r0, r1) in enumerate(clamped):
                    written[r0:r1] = True
                    if e in alone and r1 > r0:
                        dense = packed.glu_skinny(x[r0:r1], gates[e], ups[e], bias_gate=bgd[e], bias_up=bud[e], out_dtype=out_dtype, split=eff)
                        assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (rows, split, e)
                        pair = _pair_combine(x[r0:r1], gates[e], ups[e], n, "silu", bgd[e], bud[e], dtype, eff)      # the skinny pair itself
                        assert np.array_equal(_bits(out[r0:r1]), _bits(pair)), (rows, split, e)
                assert bool((out[torch.from_numpy(~written).cuda()] == -7.0).all()), (rows, "a row of no group was written")


def test_grouped_up_blob_past_its_own_groups_range_reads_as_zeros_in_that_up_projection_only():
    n, k, rows = 40, 100, (0, 5, 12, 21)
    total_rows = rows[-1]
    rng = np.random.default_rng(4243)
    x = rng.integers(-4, 5, size=(total_rows, k)).astype(np.float32)
    wg, wu = (_coarse_grid(rng.integers(-255, 256, size=(COUNT, n, k)) * 2.0 ** -8) for _ in range(2))
    bg, bu = (_coarse_grid(rng.integers(-255, 256, size=(COUNT, n)) * 2.0 ** -8) for _ in range(2))
    mg = np.stack([random_map((n, k), 140 + i) for i in range(COUNT)])
    mu = np.stack([random_map((n, k), 150 + i) for i in range(COUNT)])
    what_g, what_u = np.stack([_what(wg[i], mg[i]) for i in range(COUNT)]), np.stack([_what(wu[i], mu[i]) for i in range(COUNT)])
    gates = packed.pack_batch(torch.from_numpy(wg).cuda(), mg, backend="hip")
    ups = packed.pack_batch(torch.from_numpy(wu).cuda(), mu, backend="hip")
    e = 1
    bases = packed.batch_of(ups).bases_dev.clone()
    bases[e + 1] -= 1                                    # the up expert's stream ends one unit early: its last tile does not fit
    tiles_h, tiles_w = ups[0].map.shape
    left_u = what_u.copy()
    left_u[e] = _zeroed(what_u[e], tiles_w, [tiles_h * tiles_w - 1])
    xd, bgd, bud, r = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda(), _rows_dev(rows)
    for split in (0, 1, 2):
        got = hb.packed_glu_skinny_grouped(xd, r, _tables(gates), _tables(ups, bases_dev=bases), COUNT, n, act="none", bias_gate=bgd, bias_up=bud,
                                           split=split).cpu().numpy().astype(np.float64)
        g = hb.packed_linear_skinny_grouped(xd, r, *_tables(gates), COUNT, n, bias=bgd, split=split)
        u = hb.packed_linear_skinny_grouped(xd, r, *_tables(ups, bases_dev=bases), COUNT, n, bias=bud, split=split)
        pair = hb.glu_combine(g, u, act="none").cpu().numpy().astype(np.float64)
        for i in (0, 1):                                 # up expert 2 now starts a unit early: it reads bytes of the arena that mean nothing
            r0, r1 = rows[i], rows[i + 1]
            want = _exact_product(x[r0:r1], what_g[i], bg[i], left_u[i], bu[i])
            assert np.array_equal(got[r0:r1], want), (split, i, np.argwhere(got[r0:r1] != want)[:4])
            assert np.array_equal(pair[r0:r1], want), (split, i)
            if i == e:
                assert not np.array_equal(want, _exact_product(x[r0:r1], what_g[i], bg[i], what_u[i], bu[i]))
    assert np.array_equal(packed.batch_of(ups).bases_dev.cpu().numpy().view(np.uint64), packed.batch_of(ups).bases)


# ----------------------------------------------------------------------------- modules

def test_packed_mlp_fused_decode_equals_the_default_module():
    n, k, k_out = 96, 288, 40
    gate, up, _bg, _bu = _weights(n, k, "heavy")
    down = packed.pack(gen("heavy_f32", 91, (k_out, n)), random_map((k_out, n), 92), backend="hip")
    x = _x_dev(to_bf16_valued(gen("normal_f32", 93, (40, k)) * 8))
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            default = packed.PackedMLP(gate, up, down, act=act, out_dtype=out_dtype)
            fused = packed.PackedMLP(gate, up, down, act=act, out_dtype=out_dtype, decode_kernel="fused")
            assert default.decode_kernel == "pair" and fused.decode_kernel == "fused" and fused.backend == "hip"
            for m in (7, 32, 40):                        # inside the decode range, its last m, and the default's route above it
                y, want = fused(x[:m]), default(x[:m])
                assert tuple(y.shape) == (m, k_out) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), (act, out_dtype, m)
            h = packed.glu_skinny(x[:7], gate, up, act=act, out_dtype="bfloat16")
            assert np.array_equal(_bits(fused(x[:7])), _bits(packed.linear(h, down, out_dtype=out_dtype, kernel="auto")))
            h = packed.glu(x, gate, up, act=act, out_dtype="bfloat16", kernel="auto")
            assert np.array_equal(_bits(fused(x)), _bits(packed.linear(h, down, out_dtype=out_dtype, kernel="auto")))
            assert tuple(fused(x[:0]).shape) == (0, k_out)


def test_packed_experts_mlp_decode_route_is_its_written_out_composition():
    n, k, k_out = 40, 100, 64
    gates, ups, x, _bg, _bu = _grouped_case(n, k, 70)
    wd = np.stack([gen("heavy_f32", 95 + i, (k_out, n)) for i in range(COUNT)])
    downs = packed.pack_batch(torch.from_numpy(wd).cuda(), np.stack([random_map((k_out, n), 96 + i) for i in range(COUNT)]), backend="hip")
    for out_dtype, dtype in DTYPES:
        experts = packed.PackedExpertsMLP(gates, ups, downs, out_dtype=out_dtype, decode_max_rows=64)
        assert experts.backend == "hip" and experts.decode_max_rows == 64
        need = max(hb.packed_glu_skinny_grouped_workspace_bytes(64, COUNT, n, k), hb.packed_linear_skinny_grouped_workspace_bytes(64, COUNT, k_out, n))
        assert experts._decode_workspace.numel() == need
        rows = [0, 5, 5, 21]                             # T = 21: the decode route
        h = packed.glu_grouped_skinny(x[:21], rows, gates, ups, out_dtype="bfloat16")
        g = packed.linear_grouped(x[:21], rows, gates, out_dtype="float32", kernel="walk")             # and h is the two walks' and the combine's
        u = packed.linear_grouped(x[:21], rows, ups, out_dtype="float32", kernel="walk")
        assert np.array_equal(_bits(h), _bits(hb.glu_combine(g, u, out_dtype=torch.bfloat16)))
        want = packed.linear_grouped(h, rows, downs, out_dtype=out_dtype, kernel="walk")
        for r in (rows, _rows_dev(rows)):
            y = experts(x[:21], r)
            assert tuple(y.shape) == (21, k_out) and y.dtype == dtype and np.array_equal(_bits(y), _bits(want)), out_dtype
        rows = [0, 3, 40, 70]                            # T = 70 > decode_max_rows: the wide composition, the default module's
        h = packed.glu_grouped(x, rows, gates, ups, out_dtype="bfloat16", kernel="fused")
        want = packed.linear_grouped_wide(h, rows, downs, out_dtype=out_dtype)
        y = experts(x, rows)
        assert np.array_equal(_bits(y), _bits(want)) and np.array_equal(_bits(y), _bits(packed.PackedExpertsMLP(gates, ups, downs, out_dtype=out_dtype)(x, rows)))
        assert tuple(experts(x[:0], [0] * (COUNT + 1)).shape) == (0, k_out)
