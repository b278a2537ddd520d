"""GPU: the grouped wide matmul for (k, n) experts - packed_wide_grouped_kernel<.., WT = true> of csrc/mtq_packed.hip (wide_block fed from the
k x n stream in the grouped wide frame) - and packed.matmul_grouped_wide / PackedExpertsMatmul(wide_min_rows=...).

Routings, in 128-row blocks: (0, 3, 3, 131, 132, 390) - 6 blocks in 8 slots; (0, 0, 300, 300, 300, 300) - a hot group of 2 x 128 + 44
rows; (0, 129, 258, 387) with count = 3 - the slot bound met exactly; (0, 0, 0, 1, 1, 1) - one row.
Shapes (n, k): (72, 300) - one column block whose fourth tile column is absent, a ragged k on the element-wise X path; (200, 128) - two
column blocks, the second ragged, two K steps, the 16-byte X path; k = 64 and k = 192 on the first routing.

  * bits: == matmul(kernel="block") per group on the group's rows, both output types, with and without bias, aligned and unaligned X
    views, Y into sentinels, twice over a 0xFF workspace with sentinel bytes behind it;
  * exact arithmetic: the integer grid EQUALS float64 on the hot routing, one-hot rows return P̂[e], one flipped byte shows at its position;
  * count = 300 with groups of 0, 1 and 130 rows; the guard list of the skinny test; the module on both sides of its threshold.
The oracle for bits is never the new code."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen
from tests.packed_cases import TILE_BYTES, random_map
from tests.test_packed_grouped_gpu import _covered, _rows_dev
from tests.test_packed_long_k_gpu import _code_byte
from tests.test_packed_matmul_grouped_gpu import COUNT, DTYPES, K, N, _case, _grid_experts, _product, _ranges, _zeroed
from tests.test_packed_matmul_skinny_gpu import _bits, _phat, _same, _x_dev

pytestmark = pytest.mark.gpu

FIRST = (0, 3, 3, 131, 132, 390)
HOT = (0, 0, 300, 300, 300, 300)
ROUTINGS = {"surplus": FIRST, "hot": HOT, "exact-bound": (0, 129, 258, 387), "one-row": (0, 0, 0, 1, 1, 1)}
CASES = [(r, n, k) for r in ROUTINGS for n, k in ((72, 300), (200, 128))] + [("surplus", 72, 64), ("surplus", 200, 192)]
PAD = 16


def _blocks(rows):
    return sum(-(-(b - a) // 128) for a, b in zip(rows, rows[1:]))


def _workspace(T, count, n, k):
    """(the workspace the entry is given, the buffer it is the head of): `need` bytes of 0xFF with bytes of 0xA5 behind them."""
    need = hb.packed_matmul_wide_grouped_workspace_bytes(T, count, n, k)
    assert need == ((count + 1) * 4 + 15) // 16 * 16
    buf = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:need] = 0xFF
    return buf[:need], buf


def _wide(pts, x, rows, bias, dtype, arena=None, maps_dev=None, bases_dev=None, **kw):
    batch = packed.batch_of(pts)
    return hb.packed_matmul_wide_grouped(x, rows if torch.is_tensor(rows) else _rows_dev(rows), batch.arena if arena is None else arena,
                                         batch.maps_dev if maps_dev is None else maps_dev, batch.offsets_dev,
                                         batch.bases_dev if bases_dev is None else bases_dev, batch.count, batch.cols, bias=bias, out_dtype=dtype, **kw)


def _block_reference(pts, x, rows, bias, dtype, fill=0.0):
    """The contract's right-hand side: hb.packed_matmul (the block kernel) per group on the group's rows; `fill` in rows of no group."""
    n = pts[0].cols
    want = torch.full((x.shape[0], n), fill, dtype=dtype, device="cuda")
    for e, pt in enumerate(pts):
        r0, r1 = rows[e], rows[e + 1]
        if r1 > r0:
            want[r0:r1] = hb.packed_matmul(x[r0:r1], pt.data, pt.tables(), n, bias=None if bias is None else bias[e], out_dtype=dtype)
    return want


def _contract_holds(pts, x, bias, rows, nan=False, views=True):
    T, k = (int(v) for v in x.shape)
    count, n = len(pts), pts[0].cols
    cover = torch.from_numpy(_covered(rows, T)).cuda()
    for out_dtype, dtype in DTYPES.items():
        for b in (None, bias):
            want = _block_reference(pts, x, rows, b, dtype)
            ws, buf = _workspace(T, count, n, k)
            for twice in range(2):                           # the second call over what the first left in the workspace
                got = _wide(pts, x, rows, b, dtype, workspace=ws)
                assert tuple(got.shape) == (T, n) and got.dtype == dtype
                _same(got, want, nan, (out_dtype, b is not None, twice))
                assert bool((buf[-256:] == 0xA5).all())
            _same(_wide(pts, x, rows, b, dtype), want, nan, (out_dtype, "a workspace of its own"))
            _same(packed.matmul_grouped_wide(x, list(rows), pts, bias=b, out_dtype=out_dtype), want, nan, (out_dtype, "packed.py"))
        if not views:
            continue
        want = _block_reference(pts, x, rows, bias, dtype, fill=-7.0)
        for lead, width in ((8, k + 24), (1, k + 9)):        # 16-byte aligned rows (the 16-byte loads when k % 8 == 0); an unaligned first element
            xw = torch.full((T + PAD, width), 3.0, dtype=torch.bfloat16, device="cuda")
            xw[:T, lead:lead + k] = x
            xv = xw[:T, lead:lead + k]
            assert (xv.data_ptr() % 16 == 0 and xv.stride(0) % 8 == 0) == (lead == 8 and k % 8 == 0)
            yw = torch.full((T + PAD, n + 9), -7.0, dtype=dtype, device="cuda")
            ws, buf = _workspace(T, count, n, k)
            _wide(pts, xv, rows, bias, dtype, out=yw[:T, 5:5 + n], workspace=ws)
            _same(yw[:T, 5:5 + n].contiguous(), want, nan, (out_dtype, lead, "pitched y"))
            assert bool((yw[:, :5] == -7.0).all()) and bool((yw[:, 5 + n:] == -7.0).all()) and bool((yw[T:] == -7.0).all())
            assert bool((buf[-256:] == 0xA5).all()) and bool(cover.any())


@pytest.mark.parametrize("routing,n,k", CASES)
def test_wide_grouped_is_the_block_matmul_per_group(routing, n, k):
    rows = ROUTINGS[routing]
    count, T = len(rows) - 1, rows[-1]
    slots = (T + 127 * min(count, T)) // 128
    assert _blocks(rows) <= slots
    if routing == "surplus":
        assert [b - a for a, b in zip(rows, rows[1:])] == [3, 0, 128, 1, 258] and (_blocks(rows), slots) == (6, 8)
    if routing == "exact-bound":
        assert _blocks(rows) == slots == 6
    pts, _ref, x, _view, bias = _case(count, n, k, T, 3000 + 7 * n + k)
    _contract_holds(pts, x, bias, rows)


def test_wide_grouped_on_the_specials_weight():
    pts, _ref, x, _view, bias = _case(COUNT, N, K, FIRST[-1], 5100, "specials")
    assert not bool(torch.isfinite(_wide(pts, x, FIRST, bias, torch.float32)).all())              # the specials reach the output
    _contract_holds(pts, x, bias, FIRST, nan=True, views=False)


# ----------------------------------------------------------------------------- exact arithmetic

def test_wide_grouped_integer_grid_equals_the_float64_product():
    pts, phat, b, x = _grid_experts(COUNT, N, K, HOT[-1], 4343)
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for bias_h, bias_d in ((None, None), (b, bd)):
        want = _product(phat, bias_h, x, _ranges(HOT), HOT[-1])
        got = packed.matmul_grouped_wide(xd, list(HOT), pts, bias=bias_d).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), np.argwhere(got != want)[:4]
        half = packed.matmul_grouped_wide(xd, _rows_dev(HOT), pts, bias=bias_d, out_dtype="bfloat16")
        assert torch.equal(half.cpu(), torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))
        assert np.array_equal(packed.matmul_grouped_wide(x, list(HOT), pts, bias=bias_h, backend="emulation").astype(np.float64), want)


def test_wide_grouped_one_hot_and_a_flipped_byte():
    s, last = 3, COUNT - 1
    w = np.stack([gen("normal_f32", 820 + i, (N, K)) for i in range(COUNT)])
    maps = np.stack([random_map((K, N), 830 + i) for i in range(COUNT)])
    maps[last, -1, -1] = 1
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")          # this test's own arena: a byte of it is flipped
    rows = [0, 0, 0, 0, 0, K]
    xd = _x_dev(np.eye(K, dtype=np.float32) * np.float32(2.0 ** s))
    want = (2.0 ** s) * _phat(w[last], maps[last])
    tr, tc, r, c = maps.shape[1] - 1, maps.shape[2] - 1, 4, 5
    at, mask = _code_byte(pts[last], tr, tc, r, c)
    for flipped in (False, True):
        if flipped:
            pts[last].data[at] ^= mask
        y = packed.matmul_grouped_wide(xd, rows, pts).cpu().numpy().astype(np.float64)
        bad = np.argwhere(y != want)
        assert [tuple(v) for v in bad] == ([(32 * tr + r, 32 * tc + c)] if flipped else []), (flipped, bad[:6])


def test_wide_grouped_three_hundred_groups():
    count, n, k = 300, 40, 64
    sizes = [(0, 1, 130)[e % 3] for e in range(count)]
    rows = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    T = rows[-1]
    pts, phat, b, x = _grid_experts(count, n, k, T, 78)
    want = _product(phat, b, x, _ranges(rows), T)
    got = packed.matmul_grouped_wide(_x_dev(x.copy()), _rows_dev(rows), pts, bias=torch.from_numpy(b.copy()).cuda()).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ----------------------------------------------------------------------------- guards over buffers that stay whole

def _guarded(pts, x, b, rows, **kw):
    """The entry with sentinel rows behind X and Y and sentinel bytes behind the workspace → Y's T rows as float64; the sentinels hold."""
    batch = packed.batch_of(pts)
    T, k, n = x.shape[0], batch.rows, batch.cols
    xbuf = torch.full((T + PAD, k), 3.0, dtype=torch.bfloat16, device="cuda")
    xbuf[:T] = _x_dev(x.copy())
    ybuf = torch.full((T + PAD, n), -7.0, dtype=torch.float32, device="cuda")
    ws, buf = _workspace(T, batch.count, n, k)
    _wide(pts, xbuf[:T], rows, None if b is None else torch.from_numpy(b.copy()).cuda(), torch.float32, out=ybuf[:T], workspace=ws, **kw)
    assert bool((ybuf[T:] == -7.0).all()) and bool((buf[-256:] == 0xA5).all()) and bool((xbuf[T:] == 3.0).all())
    return ybuf[:T].cpu().numpy().astype(np.float64)


def test_wide_grouped_blobs_outside_their_stream_and_codes_that_are_no_format_multiply_as_zeros():
    rows = HOT
    pts, phat, b, x = _grid_experts(COUNT, N, K, HOT[-1], 4343)
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    tiles = tiles_h * tiles_w
    e = 1                                                    # the one group with rows
    cut = (int(batch.bases[e]) + int(pts[e].offsets[tiles - 1])) * 64 + 64
    assert COUNT * tiles * TILE_BYTES[3] <= cut < batch.arena.numel()
    short = batch.arena[:cut]                                # the buffer stays whole
    left = _zeroed(phat, e, tiles_w, [tiles - 1])
    assert np.count_nonzero(left != phat) > 0
    for bias in (None, b):
        got = _guarded(pts, x, bias, rows, arena=short)
        want = _product(left, bias, x, _ranges(rows), rows[-1], fill=-7.0)
        assert np.array_equal(got, want), ("packed_bytes", bias is not None, np.argwhere(got != want)[:4])
    bases = batch.bases_dev.clone()
    bases[e + 1] -= 1                                        # the group's own stream ends a unit early
    got = _guarded(pts, x, b, rows, bases_dev=bases)
    assert np.array_equal(got, _product(left, b, x, _ranges(rows), rows[-1], fill=-7.0)), "bases"
    assert np.array_equal(batch.bases_dev.cpu().numpy().view(np.uint64), batch.bases)
    t_first, t_second = 3 * tiles_w + 0, 9 * tiles_w + 2
    maps = batch.maps_dev.clone()
    maps[e, t_first] = 4
    maps[e, t_second] = -1
    got = _guarded(pts, x, b, rows, maps_dev=maps)
    want = _product(_zeroed(phat, e, tiles_w, (t_first, t_second)), b, x, _ranges(rows), rows[-1], fill=-7.0)
    assert np.array_equal(got, want), ("codes", np.argwhere(got != want)[:4])


T0 = FIRST[-1]
BAD_ROWS = {
    "decreasing": ([0, 3, 3, 131, 20, 20], (0, 2)),
    "overlapping": ([0, 140, 20, 150, 260, 390], (3, 4)),    # groups 0 (0..140) and 2 (20..150) overlap: their rows are unspecified
    "past-T": ([0, 3, 3, 131, 132, T0 + 9], (0, 2, 3, 4)),
    "negative": ([-5, 3, 3, 131, 132, T0], (0, 2, 3, 4)),
    "no-group": ([0, 3, 3, 10, 140, 141], (0, 2, 3, 4)),     # rows 141.. belong to no group
}


@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_wide_grouped_group_rows_are_clamped_before_any_use(name):
    rows, right = BAD_ROWS[name]
    pts, phat, b, x = _grid_experts(COUNT, N, K, T0, 4444)
    r0, r1 = packed.clamp_group_rows(rows, T0)
    written = np.zeros(T0, dtype=bool)
    for e in range(COUNT):
        written[r0[e]:r1[e]] = True
    got = _guarded(pts, x, b, rows)
    for e in right:
        want = x[r0[e]:r1[e]].astype(np.float64) @ phat[e] + b[e].astype(np.float64)[None, :]
        assert np.array_equal(got[r0[e]:r1[e]], want), (name, e)
    assert np.all(got[~written] == -7.0), (name, "a row of no clamped group was written")
    if name in ("decreasing", "overlapping"):
        return
    rows_dev = _rows_dev(rows)
    emu = packed.matmul_grouped_wide(x, rows_dev, pts, bias=b, backend="emulation")
    dev = packed.matmul_grouped_wide(_x_dev(x.copy()), rows_dev, pts, bias=torch.from_numpy(b.copy()).cuda()).cpu().numpy()
    assert np.array_equal(emu, dev) and (name != "no-group" or not emu[141:].any()), name


# ----------------------------------------------------------------------------- the module

def test_the_module_takes_the_wide_route_from_its_threshold_on(monkeypatch):
    pts, _ref, x, _view, bias = _case(COUNT, N, K, FIRST[-1], 3000 + 7 * N + K)
    mod = packed.PackedExpertsMatmul(pts, bias=bias, wide_min_rows=64)
    plan = hb.packed_matmul_wide_grouped_workspace_bytes(1, COUNT, N, K)
    assert mod._workspace is not None and mod._workspace.numel() == plan
    taken = []
    real_wide, real_skinny = packed.matmul_grouped_wide, packed.matmul_grouped
    monkeypatch.setattr(packed, "matmul_grouped_wide", lambda *a, **kw: (taken.append("wide"), real_wide(*a, **kw))[1])
    monkeypatch.setattr(packed, "matmul_grouped", lambda *a, **kw: (taken.append("skinny"), real_skinny(*a, **kw))[1])
    small = [0, 3, 3, 35, 36, 63]
    for rows, xs, route in ((list(FIRST), x, "wide"), (small, x[:63], "skinny"), ([0, 3, 3, 35, 36, 64], x[:64], "wide"), (small, x[:63], "skinny")):
        y = mod(xs, rows)
        want = (real_wide if route == "wide" else real_skinny)(xs, rows, pts, bias=bias)
        assert taken[-1] == route and torch.equal(_bits(y), _bits(want)), (route, len(xs))
    need = hb.packed_matmul_skinny_grouped_workspace_bytes(63, COUNT, N, K, 0)
    assert need > plan and mod._workspace.numel() == need   # one kept workspace: grown once, used by both routes
    ws = mod._workspace
    mod(x, list(FIRST))
    mod(x[:63], small)
    assert mod._workspace is ws
