"""GPU: the gated product on packed (k, n) weights, wide and wide-grouped — packed_glu_wide_kernel and
packed_glu_wide_grouped_kernel with WT = true of csrc/mtq_packed.hip (wide_block<GLU, .., WT>) — and packed.glu_matmul / glu_matmul_grouped.

Names: W is the (n, k) weight as stored, P̂ its packed transpose (k, n), a map is over Wᵀ's grid ceil(k/32) × ceil(n/32).

The block is 128 (M) × 64 hidden (N) × 64 (K); wave w stages hidden tile COLUMN n0 / 32 + (w >> 1) from the gate (w even) or the up
(w odd) stream, two tile ROWS of it a step.  The shapes are the smallest at which that can go wrong:

  m = 1, 33, 257, 300   one row; a second 32-row MFMA block of one row; a third row block of one row; ragged inside an MFMA block;
  n = 40                one column block whose second tile column is ragged (8 of 32);
  n = 72                a second column block whose second tile column is absent;
  n = 200               four column blocks, the last with a ragged and an absent tile column;
  k = 100               four tile rows, the last ragged; the element-wise X path;
  k = 140               FIVE tile rows: the last step's second tile row is absent (the odd count the WT table fetch branches on) and the
                        last present row is ragged; the element-wise X path;
  k = 136               the same through the 16-byte X path;
  k = 320               whole, the 16-byte X path;
  (300, 200, 2100)      33 steps, once.

Maps: the gate's random over all four codes, the up's random from another seed, and both all-bfp4.

  * bit contract: glu_matmul(kernel="fused") == glu_matmul(kernel="unfused") — two mtq_packed_matmul calls into float32 and
    mtq_glu_combine — on the words: both acts, both output types, the four bias combinations, X contiguous and at an unaligned pitch, Y
    into a pitched buffer whose sentinels stay, every call twice; heavy-tailed weights and, NaN-aware, the specials tensor; exchanging
    gate and up changes the result;
  * across the families: the result equals packed.glu(kernel="unfused") on the all-bf16 row-layout packings of unpack_transposed(P̂);
  * exact arithmetic: act="none" on the integer grid (tests/packed_cases.py, weights and biases coarsened to 2⁻⁴) EQUALS the float64
    emulation;
  * guards over buffers that stay whole: the gate's packed_bytes cut short of its last tile, map codes 4 and −1 in the up's map: zeros
    in that tile's own projection only, and the unfused route's bits under the same damage;
  * grouped, with the routings of the grouped wide tests: fused == unfused, == glu_matmul per expert, rows of no group keep what `out`
    held, a decreasing group_rows is clamped, a blob past its own group's range in the up arena reads as zeros in that expert's up
    projection only.
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
from tests.packed_cases import TILE_BYTES, random_map, specials, uniform_map
from tests.test_packed_glu_gpu import ROUTINGS, _bits, _coarse_grid, _exact_product, _grid_pair, _same, _x, _x_dev, _zeroed
from tests.test_packed_grouped_gpu import _covered, _rows_dev
from tests.test_packed_matmul_wide_gpu import _phat

pytestmark = pytest.mark.gpu
SHAPES = [(m, n, k) for m in (1, 33, 257, 300) for n in (40, 72, 200) for k in (100, 140)] + [(300, 200, 2100)]
SHAPES += [(1, 72, 136), (33, 200, 136), (257, 40, 136), (300, 72, 136), (33, 40, 320), (300, 200, 320)]   # k % 8 == 0: the 16-byte loads of X
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
ACTS = ("silu", "none")
SENTINEL = 0xA5


def _maps(n, k):
    """(name, the gate's map, the up's map), over Wᵀ's grid"""
    return (("random", random_map((k, n), n + k), random_map((k, n), n + k + 1000)), ("bfp4", uniform_map((k, n), 2), uniform_map((k, n), 2)))


@functools.lru_cache(maxsize=None)
def _weights(n, k, kind, which):
    """(P̂g, P̂u, gate bias, up bias) on the device — made once per (n, k, values, maps), never written to."""
    if kind == "specials":
        wg, wu = specials((n, k), seed=n + k), specials((n, k), seed=n + k + 5)
    else:
        wg, wu = gen("heavy_f32", 7 * n + k, (n, k)), gen("heavy_f32", 7 * n + k + 5, (n, k))
    _name, mg, mu = next(v for v in _maps(n, k) if v[0] == which)
    if which == "random":
        assert not np.array_equal(mg, mu)
    return (packed.pack_transposed(wg, mg, backend="hip"), packed.pack_transposed(wu, mu, backend="hip"),
            torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda(), torch.from_numpy(gen("normal_f32", n + 3 * k + 1, (n,))).cuda())


@functools.lru_cache(maxsize=None)
def _row_layout(n, k, kind, which):
    """The all-bf16 row-layout (n, k) packings of unpack_transposed(P̂g), unpack_transposed(P̂u)."""
    gate, up, _bg, _bu = _weights(n, k, kind, which)
    return tuple(packed.pack(packed.unpack_transposed(pt, backend="hip", dtype="bfloat16"), uniform_map((n, k), 0), backend="hip") for pt in (gate, up))


def _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype):
    """hb.packed_glu_matmul_wide into a pitched view of a buffer of sentinels → the (m, n) result; the columns and rows around it stay."""
    m = xd.shape[0]
    sentinel = -7.0
    buf = torch.full((m + 2, n + 5), sentinel, dtype=dtype, device="cuda")
    out = buf[1:1 + m, 2:2 + n]
    got = hb.packed_glu_matmul_wide(xd, gate.data, gate.tables(), up.data, up.tables(), n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = buf.float().cpu().numpy()
    inside = np.zeros(whole.shape, dtype=bool)
    inside[1:1 + m, 2:2 + n] = True
    assert np.all(whole[~inside] == sentinel), (m, n, np.argwhere((whole != sentinel) & ~inside)[:4])
    return out


def _bit_contract(m, n, k, kind, names):
    plain, pitched = _x(m, k)
    if k % 8 == 0:
        assert plain.data_ptr() % 16 == 0 and plain.stride(0) % 8 == 0        # the 16-byte X path
    nan = kind == "specials"
    for which in names:
        gate, up, bgd, bud = _weights(n, k, kind, which)
        rg, ru = _row_layout(n, k, kind, which)
        for layout, xd in (("contiguous", plain), ("pitched", pitched)):
            for act in ACTS:
                for out_dtype, dtype in DTYPES:
                    for bg, bu in ((None, None), (bgd, None), (None, bud), (bgd, bud)):
                        what = (m, n, k, kind, which, layout, act, out_dtype, bg is not None, bu is not None)
                        unfused = packed.glu_matmul(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="unfused")
                        assert tuple(unfused.shape) == (m, n) and unfused.dtype == dtype
                        y = packed.glu_matmul(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="fused")
                        assert tuple(y.shape) == (m, n) and y.dtype == dtype
                        _same(y, unfused, nan, what)
                        first = _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype)
                        _same(first, unfused, nan, what)
                        again = _fused_into_sentinels(xd, gate, up, n, act, bg, bu, dtype)
                        assert np.array_equal(_bits(again), _bits(first)), what
                        if layout == "contiguous":           # across the families: the linear GLU on the transposed weight
                            lin = packed.glu(xd, rg, ru, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="unfused")
                            _same(y, lin, nan, what + ("the linear family",))
        if kind == "heavy":                              # the streams are told apart: exchanged, the result changes
            for act in ACTS:
                there = packed.glu_matmul(plain, gate, up, act=act, bias_gate=bgd, kernel="fused")
                back = packed.glu_matmul(plain, up, gate, act=act, bias_gate=bgd, kernel="fused")
                assert not np.array_equal(_bits(there), _bits(back)), (m, n, k, which, act)
                _same(back, packed.glu_matmul(plain, up, gate, act=act, bias_gate=bgd, kernel="unfused"), False, (m, n, k, which, act, "exchanged"))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_fused_is_the_unfused_route_bit_for_bit(m, n, k):
    _bit_contract(m, n, k, "heavy", ("random", "bfp4"))


@pytest.mark.parametrize("m,n,k", [s for s in SHAPES if s[2] <= 320])
def test_fused_is_the_unfused_route_on_specials(m, n, k):
    _bit_contract(m, n, k, "specials", ("random",))
    gate, up, _bg, _bu = _weights(n, k, "specials", "random")
    y = packed.glu_matmul(_x(m, k)[0], gate, up, kernel="fused")
    assert m * n < 200 or not bool(torch.isfinite(y).all())                  # the specials reach the output


def test_auto_takes_the_route_its_constants_name():
    n, k = 72, 140
    gate, up, bgd, bud = _weights(n, k, "heavy", "random")
    for m in (1, 32, 33, 63, 64, 257):
        xd = _x_dev(to_bf16_valued(gen("normal_f32", 5 + m, (m, k)) * 40))
        y = packed.glu_matmul(xd, gate, up, bias_gate=bgd, bias_up=bud, kernel="auto")
        if packed.AUTO_GLU_MATMUL_SKINNY_MAX_M is not None and m <= packed.AUTO_GLU_MATMUL_SKINNY_MAX_M:
            g = packed.matmul(xd, gate, bias=bgd, kernel="skinny")
            u = packed.matmul(xd, up, bias=bud, kernel="skinny")
            want = hb.glu_combine(g, u)
        else:                                            # fused or unfused: the same bits
            want = packed.glu_matmul(xd, gate, up, bias_gate=bgd, bias_up=bud, kernel="unfused")
        assert np.array_equal(_bits(y), _bits(want)), m
    for kernel in packed.GLU_KERNELS:
        assert tuple(packed.glu_matmul(xd[:0], gate, up, kernel=kernel).shape) == (0, n)


# ----------------------------------------------------------------------------- exact arithmetic, independent of the block kernel

def _what_t(w, amap):
    """unpack(P̂)ᵀ (n, k) as float64, from the oracle."""
    return np.ascontiguousarray(_phat(w, amap).T)


@pytest.mark.parametrize("m,n,k", [(300, 200, 140), (257, 72, 2100), (300, 200, 320), (33, 40, 136)])
def test_act_none_on_the_integer_grid_equals_the_float64_emulation(m, n, k):
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 1000 * m + 10 * n + k)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda()
    zero = np.zeros(n, dtype=np.float32)
    for which, mg, mu in _maps(n, k):
        what_g, what_u = _what_t(wg, mg), _what_t(wu, mu)
        gate, up = packed.pack_transposed(wg, mg, backend="hip"), packed.pack_transposed(wu, mu, backend="hip")
        for b_g, b_u, d_g, d_u in ((bg, bu, bgd, bud), (zero, bu, None, bud), (bg, zero, bgd, None), (zero, zero, None, None)):
            want = _exact_product(x, what_g, b_g, what_u, b_u)
            emu = packed.glu_matmul(x, gate, up, act="none", bias_gate=None if d_g is None else b_g, bias_up=None if d_u is None else b_u,
                                    backend="emulation")
            assert np.array_equal(emu.astype(np.float64), want)
            for kernel in ("fused", "unfused"):
                got = packed.glu_matmul(xd, gate, up, act="none", bias_gate=d_g, bias_up=d_u, kernel=kernel).cpu().numpy()
                assert got.shape == (m, n) and got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), want), (m, n, k, which, kernel, np.argwhere(got != want)[:4])
        half = packed.glu_matmul(xd, gate, up, act="none", bias_gate=bgd, bias_up=bud, out_dtype="bfloat16", kernel="fused")
        want = _exact_product(x, what_g, bg, what_u, bu)
        assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))), (m, n, k, which)


# ----------------------------------------------------------------------------- blobs that are not there

@functools.lru_cache(maxsize=None)
def _guard_case():
    m, n, k = 300, 200, 300
    x, wg, bg, wu, bu = _grid_pair(m, n, k, 77)
    mg, mu = random_map((k, n), 78), random_map((k, n), 79)
    return (n, x, packed.pack_transposed(wg, mg, backend="hip"), _phat(wg, mg), bg, packed.pack_transposed(wu, mu, backend="hip"), _phat(wu, mu),
            bu)


def _guarded(gate_tables, up_tables, gone_gate, gone_up):
    """Through the given tables: the unfused route's bits under the same damage, and (act none, float32) the exact product with the tiles
    `gone_*` (numbered in the k × n grid) as zeros in their own projection only.  The streams are whole: a kernel without the guard reads
    real bytes and fails."""
    n, x, gate, phat_g, bg, up, phat_u, bu = _guard_case()
    for pt in (gate, up):
        assert pt.data.numel() == pt.nbytes == pt.tables().nbytes            # never a shorter buffer
    left_g, left_u = _zeroed(phat_g, gate.map.shape[1], gone_gate), _zeroed(phat_u, up.map.shape[1], gone_up)
    assert (np.count_nonzero(left_g != phat_g) > 0) == bool(gone_gate) and (np.count_nonzero(left_u != phat_u) > 0) == bool(gone_up)
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg.copy()).cuda(), torch.from_numpy(bu.copy()).cuda()
    want = _exact_product(x, np.ascontiguousarray(left_g.T), bg, np.ascontiguousarray(left_u.T), bu)
    assert not np.array_equal(want, _exact_product(x, np.ascontiguousarray(phat_g.T), bg, np.ascontiguousarray(phat_u.T), bu))
    for act in ACTS:
        for dtype in (torch.float32, torch.bfloat16):
            g = hb.packed_matmul(xd, gate.data, gate_tables, n, bias=bgd, out_dtype=torch.float32)
            u = hb.packed_matmul(xd, up.data, up_tables, n, bias=bud, out_dtype=torch.float32)
            unfused = hb.glu_combine(g, u, act=act, out_dtype=dtype)
            y = hb.packed_glu_matmul_wide(xd, gate.data, gate_tables, up.data, up_tables, n, act=act, bias_gate=bgd, bias_up=bud, out_dtype=dtype)
            assert np.array_equal(_bits(y), _bits(unfused)), (act, dtype)
            if act == "none" and dtype == torch.float32:
                got = y.cpu().numpy().astype(np.float64)
                assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_a_gate_blob_past_its_packed_bytes_reads_as_zeros_in_the_gate_only():
    _n, _x_, gate, _pg, _bg, up, _pu, _bu = _guard_case()
    last = gate.map.size - 1
    cut = int(gate.offsets[last]) * 64 + TILE_BYTES[int(gate.map.reshape(-1)[last])] - 64      # 64 bytes short of the end of the last tile
    assert gate.map.size * TILE_BYTES[3] <= cut < gate.nbytes                # the entries refuse less
    short = copy.copy(gate.tables())                                         # the same device map and offsets, a smaller packed_bytes
    short.nbytes = cut
    _guarded(short, up.tables(), (last,), ())
    assert gate.tables().nbytes == gate.nbytes                               # the shared tables were not touched


def test_up_tiles_whose_map_code_is_no_format_read_as_zeros_in_the_up_only():
    _n, _x_, gate, _pg, _bg, up, _pu, _bu = _guard_case()
    tiles_h, tiles_w = up.map.shape                                          # 10 tile rows (k), 7 tile columns (n)
    tables = hb.PackedTables.on_device(up.map, up.offsets)                   # a private copy
    inner = (3 * tiles_w + 1, 6 * tiles_w + 5)                               # first column block, second K step; third column block, fourth K step
    assert all(0 < t // tiles_w < tiles_h - 1 and 0 < t % tiles_w < tiles_w - 1 for t in inner)
    tables.map_dev[inner[0]] = 4
    tables.map_dev[inner[1]] = -1
    _guarded(gate.tables(), tables, (), inner)
    assert np.array_equal(up.tables().map_dev.cpu().numpy(), up.map.reshape(-1))


# ----------------------------------------------------------------------------- grouped

GROUPED_CASES = [(r, n, k) for r in ROUTINGS for n, k in ((72, 140), (200, 128))]


@functools.lru_cache(maxsize=None)
def _experts(count, n, k, seed):
    """`count` (k, n) experts of one device arena, of other weights and maps per expert."""
    w = np.stack([gen("heavy_f32", seed + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((k, n), seed + 100 + i) for i in range(count)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")
    batch = packed.batch_of(pts)
    assert batch is not None and (batch.rows, batch.cols) == (k, n)
    return pts


@functools.lru_cache(maxsize=None)
def _grouped_case(count, n, k, total_rows):
    """(gate experts, up experts, x, gate bias, up bias): two arenas of other weights and maps, one X."""
    x = _x_dev(to_bf16_valued(gen("normal_f32", 3200 + 7 * n + k, (total_rows, k)) * 8))
    bg, bu = (torch.from_numpy(gen("normal_f32", s + 7 * n + k, (count, n))).cuda() for s in (3201, 4201))
    return _experts(count, n, k, 3000 + 7 * n + k), _experts(count, n, k, 4000 + 7 * n + k), x, bg, bu


def _workspace(total_rows, count, n, k):
    need = hb.packed_glu_matmul_wide_grouped_workspace_bytes(total_rows, count, n, k)
    assert need == hb.packed_glu_wide_grouped_workspace_bytes(total_rows, count, n, k)
    buf = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[:need] = 0xFF
    return buf[:need], buf


def _tables(pts, bases_dev=None):
    b = packed.batch_of(pts)
    return b.arena, b.maps_dev, b.offsets_dev, b.bases_dev if bases_dev is None else bases_dev


@pytest.mark.parametrize("routing,n,k", GROUPED_CASES)
def test_grouped_fused_is_unfused_and_the_dense_route_per_expert(routing, n, k):
    rows = ROUTINGS[routing]
    count, total_rows = len(rows) - 1, rows[-1]
    assert count in (3, 5)
    gates, ups, x, bgd, bud = _grouped_case(count, n, k, total_rows)
    covered = _covered(rows, total_rows)
    for act in ACTS:
        for out_dtype, dtype in DTYPES:
            for bg, bu in ((None, None), (bgd, None), (None, bud), (bgd, bud)):
                what = (routing, n, k, act, out_dtype, bg is not None, bu is not None)
                unfused = packed.glu_matmul_grouped(x, list(rows), gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="unfused")
                ws, buf = _workspace(total_rows, count, n, k)
                for r in (list(rows), _rows_dev(rows)):      # the second call over what the first left in the workspace
                    y = packed.glu_matmul_grouped(x, r, gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="fused",
                                                  workspace=ws)
                    assert tuple(y.shape) == (total_rows, n) and y.dtype == dtype
                    assert np.array_equal(_bits(y)[covered], _bits(unfused)[covered]), what
                    assert not bool(y[torch.from_numpy(~covered).cuda()].any())
                    assert bool((buf[-256:] == SENTINEL).all())
                for e in range(count):
                    r0, r1 = rows[e], rows[e + 1]
                    if r1 > r0:
                        dense = packed.glu_matmul(x[r0:r1], gates[e], ups[e], act=act, bias_gate=None if bg is None else bg[e],
                                                  bias_up=None if bu is None else bu[e], out_dtype=out_dtype, kernel="unfused")
                        assert np.array_equal(_bits(y[r0:r1]), _bits(dense)), (what, e)


def test_grouped_rows_of_no_group_keep_what_out_held_and_bad_rows_are_clamped():
    n, k, total_rows = 72, 140, 200
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
            got = hb.packed_glu_matmul_wide_grouped(xbuf[:total_rows], _rows_dev(rows), _tables(gates), _tables(ups), 3, n, bias_gate=bgd,
                                                    bias_up=bud, out_dtype=dtype, out=out, workspace=ws)
            assert got.data_ptr() == out.data_ptr()
            assert bool((ybuf[total_rows:] == -7.0).all()) and bool((ybuf[:, :2] == -7.0).all()) and bool((ybuf[:, 2 + n:] == -7.0).all())
            assert bool((wbuf[-256:] == SENTINEL).all())
            written = np.zeros(total_rows, dtype=bool)
            for e, (r0, r1) in enumerate(clamped):
                written[r0:r1] = True
                if r1 > r0:
                    dense = packed.glu_matmul(x[r0:r1], gates[e], ups[e], bias_gate=bgd[e], bias_up=bud[e], out_dtype=out_dtype, kernel="unfused")
                    assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (rows, e)
            assert bool((out[torch.from_numpy(~written).cuda()] == -7.0).all()), (rows, "a row of no group was written")


def test_grouped_up_blob_past_its_own_groups_range_reads_as_zeros_in_that_up_projection_only():
    count, n, k, rows = 5, 72, 140, (0, 130, 130, 162, 163, 300)
    total_rows = rows[-1]
    rng = np.random.default_rng(4243)
    x = rng.integers(-4, 5, size=(total_rows, k)).astype(np.float32)
    wg, wu = (_coarse_grid(rng.integers(-255, 256, size=(count, n, k)) * 2.0 ** -8) for _ in range(2))
    bg, bu = (_coarse_grid(rng.integers(-255, 256, size=(count, n)) * 2.0 ** -8) for _ in range(2))
    mg = np.stack([random_map((k, n), 140 + i) for i in range(count)])
    mu = np.stack([random_map((k, n), 150 + i) for i in range(count)])
    what_g = np.stack([_what_t(wg[i], mg[i]) for i in range(count)])          # (count, n, k)
    phat_u = np.stack([_phat(wu[i], mu[i]) for i in range(count)])            # (count, k, n)
    gates = packed.pack_batch_transposed(torch.from_numpy(wg).cuda(), mg, backend="hip")
    ups = packed.pack_batch_transposed(torch.from_numpy(wu).cuda(), mu, backend="hip")
    e = 2
    bases = packed.batch_of(ups).bases_dev.clone()
    bases[e + 1] -= 1                                    # the up expert's stream ends one unit early: its last tile does not fit
    tiles_h, tiles_w = ups[0].map.shape
    left_u = phat_u.copy()
    left_u[e] = _zeroed(phat_u[e], tiles_w, [tiles_h * tiles_w - 1])
    xd, bgd, bud = _x_dev(x), torch.from_numpy(bg).cuda(), torch.from_numpy(bu).cuda()
    got = hb.packed_glu_matmul_wide_grouped(xd, _rows_dev(rows), _tables(gates), _tables(ups, bases_dev=bases), count, n, act="none",
                                            bias_gate=bgd, bias_up=bud).cpu().numpy().astype(np.float64)
    g = hb.packed_matmul_wide_grouped(xd, _rows_dev(rows), *_tables(gates), count, n, bias=bgd)
    u = hb.packed_matmul_wide_grouped(xd, _rows_dev(rows), *_tables(ups, bases_dev=bases), count, n, bias=bud)
    unfused = hb.glu_combine(g, u, act="none").cpu().numpy().astype(np.float64)
    for i in (0, 1, 2, 4):                               # up expert 3 now starts a unit early: it reads bytes of the arena that mean nothing
        r0, r1 = rows[i], rows[i + 1]
        if r1 == r0:
            continue
        want = _exact_product(x[r0:r1], what_g[i], bg[i], np.ascontiguousarray(left_u[i].T), bu[i])
        assert np.array_equal(got[r0:r1], want), (i, np.argwhere(got[r0:r1] != want)[:4])
        assert np.array_equal(unfused[r0:r1], want), i
        if i == e:
            assert not np.array_equal(want, _exact_product(x[r0:r1], what_g[i], bg[i], np.ascontiguousarray(phat_u[i].T), bu[i]))
    assert np.array_equal(packed.batch_of(ups).bases_dev.cpu().numpy().view(np.uint64), packed.batch_of(ups).bases)
