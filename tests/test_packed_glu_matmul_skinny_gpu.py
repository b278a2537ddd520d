"""GPU: the gated product on packed (k, n) weights for decode — packed_glu_matmul_skinny_kernel and
packed_glu_matmul_skinny_grouped_kernel of csrc/mtq_packed.hip (skinny_run with FeedTransposed on the projection axis), finished by the
linear family's reduce kernels — and packed.glu_matmul_skinny / glu_matmul_grouped_skinny.

A unit is (slice, projection, tile column): a wave walks the tile rows of its slice through two wave-private [32 k][32 n] images.

  m = 1, 16, 32         one row, a half chunk, a whole chunk;
  n = 40, 200           two tile columns (the second ragged): 4 units a slice, one workgroup; seven: 14 units, no multiple of 4;
  k = 100, 140, 320     four tile rows, the last ragged; five, odd (the two images alternate unevenly); ten, whole, the 16-byte X path;
  split = 0, 1, 2, 3 and 1000 (clamped to the tile-row count).

  * bit contract: at every split the result equals two matmul(kernel="skinny") calls into float32 at that split and glu_combine, both
    acts, both output types, the four bias combinations, every call twice; and equals glu_skinny at that split on the all-bf16
    row-layout packings of unpack_transposed(P̂); exchanging gate and up changes the result;
  * grouped: 1, 4 and 32 rows per expert, a 70-row group walked in three chunks, empty groups, rows of no group; Y in a buffer of
    sentinels and the workspace between sentinels; == the two matmul_grouped walks and the combine, == glu_matmul_skinny per chunk at
    the effective split, == glu_grouped_skinny on the row-layout arena;
  * a workspace that is too short or misaligned is refused, at split 1 too.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map, uniform_map
from tests.test_packed_glu_gpu import _bits, _x_dev
from tests.test_packed_grouped_gpu import _rows_dev

pytestmark = pytest.mark.gpu
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
ACTS = ("silu", "none")
SPLITS = (0, 1, 2, 3, 1000)
SENTINEL = 0xA5


def _eff(m, n, k, split):
    """The effective split, from the workspace the library asks for: 2 · split_eff · m · n floats rounded up to 16 bytes."""
    need = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, split)
    assert need == hb.packed_glu_skinny_workspace_bytes(m, n, k, split)
    assert need >= 2 * 4 * m * n and (m * n * 8 < 16 or need % (8 * m * n) < 16)
    return max(1, need // (8 * m * n))


@functools.lru_cache(maxsize=None)
def _weights(n, k):
    """(P̂g, P̂u, their all-bf16 row-layout counterparts, gate bias, up bias) on the device — made once, never written to."""
    wg, wu = gen("heavy_f32", 7 * n + k, (n, k)), gen("heavy_f32", 7 * n + k + 5, (n, k))
    mg, mu = random_map((k, n), n + k), random_map((k, n), n + k + 1000)
    mg.reshape(-1)[:4], mu.reshape(-1)[:4] = [0, 1, 2, 3], [3, 2, 1, 0]      # every code in both maps, in another order
    gate, up = packed.pack_transposed(wg, mg, backend="hip"), packed.pack_transposed(wu, mu, backend="hip")
    rows = tuple(packed.pack(packed.unpack_transposed(pt, backend="hip", dtype="bfloat16"), uniform_map((n, k), 0), backend="hip") for pt in (gate, up))
    return (gate, up, rows[0], rows[1], torch.from_numpy(gen("normal_f32", n + 3 * k, (n,))).cuda(),
            torch.from_numpy(gen("normal_f32", n + 3 * k + 1, (n,))).cuda())


@functools.lru_cache(maxsize=None)
def _x(m, k):
    return _x_dev(to_bf16_valued(gen("normal_f32", 61 + m + k, (m, k)) * 8))


def _fused(xd, gate, up, n, act, bg, bu, dtype, split, **kw):
    return hb.packed_glu_matmul_skinny(xd, gate.data, gate.tables(), up.data, up.tables(), n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype,
                                       split=split, **kw)


@pytest.mark.parametrize("k", (100, 140, 320))
@pytest.mark.parametrize("n", (40, 200))
@pytest.mark.parametrize("m", (1, 16, 32))
def test_fused_is_the_skinny_pair_and_the_combine_and_the_linear_family_bit_for_bit(m, n, k):
    xd = _x(m, k)
    gate, up, rg, ru, bgd, bud = _weights(n, k)
    tiles_k = (k + 31) // 32
    for split in SPLITS:
        eff = _eff(m, n, k, split)
        assert eff == min(tiles_k, split) if split else eff == max(1, min(2048 // ((n + 31) // 32), tiles_k // 4))
        for has_g in (False, True):
            for has_u in (False, True):
                bg, bu = bgd if has_g else None, bud if has_u else None
                g = packed.matmul(xd, gate, bias=bg, kernel="skinny", split=split)
                u = packed.matmul(xd, up, bias=bu, kernel="skinny", split=split)
                for act in ACTS:
                    for out_dtype, dtype in DTYPES:
                        what = (m, n, k, split, act, out_dtype, has_g, has_u)
                        want = hb.glu_combine(g, u, act=act, out_dtype=dtype)
                        y = _fused(xd, gate, up, n, act, bg, bu, dtype, split)
                        assert tuple(y.shape) == (m, n) and y.dtype == dtype
                        assert np.array_equal(_bits(y), _bits(want)), (what, np.argwhere(_bits(y) != _bits(want))[:4])
                        assert np.array_equal(_bits(_fused(xd, gate, up, n, act, bg, bu, dtype, split)), _bits(want)), (what, "again")
                        lin = packed.glu_skinny(xd, rg, ru, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, split=split)
                        assert np.array_equal(_bits(y), _bits(lin)), (what, "the linear family")
                        if split == 0:
                            auto = packed.glu_matmul(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, kernel="auto")
                            top = packed.glu_matmul_skinny(xd, gate, up, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype)
                            assert np.array_equal(_bits(auto), _bits(want)) and np.array_equal(_bits(top), _bits(want)), what
    there = _fused(xd, gate, up, n, "silu", bgd, None, torch.float32, 0)     # the streams are told apart: exchanged, the result changes
    back = _fused(xd, up, gate, n, "silu", bgd, None, torch.float32, 0)
    assert not np.array_equal(_bits(there), _bits(back)), (m, n, k)


def _workspace(need):
    """(a slice of exactly `need` bytes, the sentinel-filled allocation around it)"""
    buf = torch.full((256 + need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = buf[256:256 + need]
    assert ws.data_ptr() % 16 == 0
    return ws, buf


def _untouched_around(buf, need):
    return bool((buf[:256] == SENTINEL).all()) and bool((buf[256 + need:] == SENTINEL).all())


@pytest.mark.parametrize("m,n,k", [(5, 40, 100), (21, 200, 140)])
def test_nothing_outside_y_or_the_workspace_is_written_and_x_may_be_pitched(m, n, k):
    xd = _x(m, k)
    gate, up, _rg, _ru, bgd, bud = _weights(n, k)
    xbuf = torch.full((m + 3, k + 9), 3.0, dtype=torch.bfloat16, device="cuda")          # rows past m and columns past k hold 3.0
    xbuf[:m, 1:1 + k] = xd
    view = xbuf[:m, 1:1 + k]
    assert view.data_ptr() % 16 != 0                     # the element-wise loads of X
    for split in SPLITS:
        need = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, split)
        for act in ACTS:
            for _name, dtype in DTYPES:
                want = _fused(xd, gate, up, n, act, bgd, bud, dtype, split)   # on the contiguous x
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
    need = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, 1)           # at split 1 too
    with pytest.raises(hb.MtqError, match="workspace"):
        _fused(xd, gate, up, n, "silu", None, None, torch.float32, 1, workspace=torch.empty((need - 16,), dtype=torch.uint8, device="cuda"))
    with pytest.raises(hb.MtqError, match="16-byte aligned"):
        _fused(xd, gate, up, n, "silu", None, None, torch.float32, 1, workspace=torch.empty((need + 16,), dtype=torch.uint8, device="cuda")[8:])
    with pytest.raises(hb.MtqError, match="m <= 32"):
        packed.glu_matmul_skinny(torch.zeros((33, k), dtype=torch.bfloat16, device="cuda"), gate, up)
    assert tuple(packed.glu_matmul_skinny(xd[:0], gate, up).shape) == (0, n)


# ----------------------------------------------------------------------------- grouped

COUNT = 3
GROUPED_SHAPES = ((40, 100), (200, 140))
# (group_rows, total_rows): 1, 4 and 32 rows per expert; an empty group; one group of 70 rows (three chunks, the last of 6) between two
# empty ones; rows 0..3 and 25..29 of no group
ROUTINGS = {"one": ((0, 1, 2, 3), 3), "four": ((0, 4, 8, 12), 12), "chunk": ((0, 32, 64, 96), 96), "empty": ((0, 5, 5, 21), 21),
            "hot": ((0, 0, 70, 70), 70), "uncovered": ((4, 9, 9, 25), 30)}


@functools.lru_cache(maxsize=None)
def _experts(n, k, seed):
    """(COUNT (k, n) experts of one device arena, the arena of all-bf16 row-layout packings of unpack(P̂[e])ᵀ)"""
    w = np.stack([gen("heavy_f32", seed + i, (n, k)) for i in range(COUNT)])
    maps = np.stack([random_map((k, n), seed + 100 + i) for i in range(COUNT)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")
    back = packed.unpack_batch_transposed(pts, backend="hip", dtype="bfloat16")                  # (count, n, k)
    return pts, packed.pack_batch(back, np.stack([uniform_map((n, k), 0)] * COUNT), backend="hip")


@functools.lru_cache(maxsize=None)
def _grouped_case(n, k, total_rows):
    x = _x_dev(to_bf16_valued(gen("normal_f32", 3200 + 7 * n + k + total_rows, (total_rows, k)) * 8))
    bg, bu = (torch.from_numpy(gen("normal_f32", s + 7 * n + k, (COUNT, n))).cuda() for s in (3201, 4201))
    return _experts(n, k, 3000 + 7 * n + k), _experts(n, k, 4000 + 7 * n + k), x, bg, bu


def _tables(pts):
    b = packed.batch_of(pts)
    return b.arena, b.maps_dev, b.offsets_dev, b.bases_dev


def _grouped_into_sentinels(x, rows_dev, gates, ups, n, act, bg, bu, dtype, split, total_rows, k):
    need = hb.packed_glu_matmul_skinny_grouped_workspace_bytes(total_rows, COUNT, n, k, split)
    assert need == hb.packed_glu_skinny_grouped_workspace_bytes(total_rows, COUNT, n, k, split)
    eff = max(1, need // (8 * total_rows * n))
    ws, wbuf = _workspace(need)
    ybuf = torch.full((total_rows + 3, n + 4), -7.0, dtype=dtype, device="cuda")
    out = ybuf[:total_rows, 2:2 + n]
    got = hb.packed_glu_matmul_skinny_grouped(x, rows_dev, _tables(gates), _tables(ups), COUNT, n, act=act, bias_gate=bg, bias_up=bu,
                                              out_dtype=dtype, out=out, split=split, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    assert bool((ybuf[total_rows:] == -7.0).all()) and bool((ybuf[:, :2] == -7.0).all()) and bool((ybuf[:, 2 + n:] == -7.0).all())
    assert _untouched_around(wbuf, need)
    return out, eff, ws


@pytest.mark.parametrize("n,k", GROUPED_SHAPES)
@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_grouped_is_the_two_walks_and_the_combine_and_the_dense_call_per_chunk(routing, n, k):
    rows, total_rows = ROUTINGS[routing]
    (gates, gates_rows), (ups, ups_rows), x, bgd, bud = _grouped_case(n, k, total_rows)
    covered = np.zeros(total_rows, dtype=bool)
    for e in range(COUNT):
        covered[rows[e]:rows[e + 1]] = True
    keep = torch.from_numpy(~covered).cuda()
    r = _rows_dev(rows)
    for split in (0, 1, 2, 1000):
        for with_bias in (False, True):
            bg, bu = (bgd, bud) if with_bias else (None, None)
            g = packed.matmul_grouped(x, r, gates, bias=bg, out_dtype="float32", split=split, kernel="walk")
            u = packed.matmul_grouped(x, r, ups, bias=bu, out_dtype="float32", split=split, kernel="walk")
            for act in ACTS:
                for out_dtype, dtype in DTYPES:
                    what = (routing, n, k, split, with_bias, act, out_dtype)
                    want = hb.glu_combine(g, u, act=act, out_dtype=dtype)
                    out, eff, ws = _grouped_into_sentinels(x, r, gates, ups, n, act, bg, bu, dtype, split, total_rows, k)
                    assert np.array_equal(_bits(out)[covered], _bits(want)[covered]), what
                    assert bool((out[keep] == -7.0).all()), (what, "a row of no group was written")
                    top = packed.glu_matmul_grouped_skinny(x, r, gates, ups, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, split=split,
                                                           workspace=ws)            # again, over what the first call left there
                    assert np.array_equal(_bits(top)[covered], _bits(want)[covered]) and not bool(top[keep].any()), what
                    lin = packed.glu_grouped_skinny(x, r, gates_rows, ups_rows, act=act, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, split=split)
                    assert np.array_equal(_bits(top), _bits(lin)), (what, "the linear family")
                    if act == "silu" or split == 0:
                        for e in range(COUNT):           # the dense call on every 32-row chunk of every group, at the effective split
                            for r0 in range(rows[e], rows[e + 1], 32):
                                r1 = min(r0 + 32, rows[e + 1])
                                dense = packed.glu_matmul_skinny(x[r0:r1], gates[e], ups[e], act=act, bias_gate=None if bg is None else bg[e],
                                                                 bias_up=None if bu is None else bu[e], out_dtype=out_dtype, split=eff)
                                assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (what, e, r0)
    if routing == "empty":                               # a checked host array gives the same call
        host = packed.glu_matmul_grouped_skinny(x, list(rows), gates, ups, bias_gate=bgd, bias_up=bud)
        assert np.array_equal(_bits(host), _bits(packed.glu_matmul_grouped_skinny(x, r, gates, ups, bias_gate=bgd, bias_up=bud)))
        assert tuple(packed.glu_matmul_grouped_skinny(x[:0], [0] * (COUNT + 1), gates, ups).shape) == (0, n)


def test_grouped_decreasing_rows_are_clamped_and_a_bad_workspace_is_refused():
    n, k, total_rows = 40, 100, 30
    (gates, _gr), (ups, _ur), x, bgd, bud = _grouped_case(n, k, total_rows)
    # (group_rows, the clamped ranges the kernel makes of them, the groups that overlap no other)
    cases = (((10, 30, 0, 8), [(10, 30), (30, 30), (0, 8)], (0, 2)),
             ((0, 21, 9, 9), [(0, 21), (21, 21), (9, 9)], (0,)),
             ((-5, 12, 12, total_rows + 9), [(0, 12), (12, 12), (12, 30)], (0, 2)))
    for rows, clamped, alone in cases:
        for e, (r0, r1) in enumerate(clamped):           # the rule, restated
            assert r0 == min(max(rows[e], 0), total_rows) and r1 == min(max(rows[e + 1], r0), total_rows)
        for split in (0, 2):
            for out_dtype, dtype in DTYPES:
                xbuf = torch.full((total_rows + 16, k), 3.0, dtype=torch.bfloat16, device="cuda")
                xbuf[:total_rows] = x
                out, eff, _ws = _grouped_into_sentinels(xbuf[:total_rows], _rows_dev(rows), gates, ups, n, "silu", bgd, bud, dtype, split, total_rows, k)
                written = np.zeros(total_rows, dtype=bool)
                for e, (r0, r1) in enumerate(clamped):
                    written[r0:r1] = True
                    if e in alone and r1 > r0:
                        dense = packed.glu_matmul_skinny(x[r0:r1], gates[e], ups[e], bias_gate=bgd[e], bias_up=bud[e], out_dtype=out_dtype, split=eff)
                        assert np.array_equal(_bits(out[r0:r1]), _bits(dense)), (rows, split, e)
                assert bool((out[torch.from_numpy(~written).cuda()] == -7.0).all()), (rows, "a row of no group was written")
    need = hb.packed_glu_matmul_skinny_grouped_workspace_bytes(total_rows, COUNT, n, k, 1)
    r = _rows_dev((0, 10, 20, 30))
    with pytest.raises(hb.MtqError, match="workspace"):
        packed.glu_matmul_grouped_skinny(x, r, gates, ups, split=1, workspace=torch.empty((need - 16,), dtype=torch.uint8, device="cuda"))
    with pytest.raises(hb.MtqError, match="16-byte aligned"):
        packed.glu_matmul_grouped_skinny(x, r, gates, ups, split=1, workspace=torch.empty((need + 16,), dtype=torch.uint8, device="cuda")[8:])
