"""GPU: the grouped wide packed linear (packed_grouped_plan_kernel<128> + packed_wide_grouped_kernel<.., WT = false> of csrc/mtq_packed.hip): a
workgroup per (128-row block of a group, 128 columns), the block list made from group_rows on the device.

The oracle for bits is never the new code: the block kernel (hb.packed_linear) per group, the float64 emulation on the integer grid, the
oracle's Ŵ under one-hot activations.

The main cases have count = 5 experts (3 for the routing that meets the bound) and a different random map per expert.  The routings:

  (0, 3, 3, 131, 132, 390)     T = 390  groups of 3, 0, 128, 1 and 258 rows: 6 blocks in 8 slots, so surplus workgroups run
  (0, 0, 300, 300, 300, 300)   T = 300  one hot group of 2 × 128 + 44 rows, empty groups around it
  (0, 129, 258, 387), count 3  T = 387  6 blocks in 6 slots: the bound met exactly, every slot used
  (0, 0, 0, 1, 1, 1)           T = 1    one row, one block, one slot

n = 72 is one column block whose fourth tile row is absent, n = 200 two column blocks, the second ragged; k = 64 is one step, 128 two
steps on the 16-byte X path, 192 three steps, 300 five steps with a ragged k on the element-wise path.  Every routing runs at (72, 300)
and (200, 128), the other (n, k) pairs on the first routing.

  * bits: float32 and bf16, with and without bias, == the block kernel per group on the words; X contiguous and as views of wider
    buffers (16-byte aligned rows, and an unaligned first element), Y into a pitched buffer of sentinels, every call over a workspace
    of 0xFF bytes with sentinels behind it, twice; the specials tensor (Inf, NaN, denormals) as weights on the first routing;
  * exact arithmetic: the integer grid on the hot routing EQUALS the float64 emulation; one-hot activations against the oracle's Ŵ, and
    one flipped code byte of the last expert's last tile shows at exactly its position;
  * count = 300 with groups of 0, 1 and 130 rows in turn takes the plan kernel past one entry per thread and the search into its bisection;
  * guards over buffers that stay whole, with sentinel rows behind X, Y and the workspace: packed_bytes cut short, a group's stream cut
    short by its own bases, map codes 4 and −1, group_rows that decrease, overlap, end at T + 9 or start below 0, and rows of no group;
  * PackedExperts(wide_min_rows=64) on both sides of its threshold, on one kept workspace.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import TILE_BYTES, _grid_preconditions, random_map, specials
from tests.test_packed_grouped_gpu import DTYPES, _case, _covered, _grid_experts, _grid_want, _rows_dev, _zeroed
from tests.test_packed_long_k_gpu import _code_byte
from tests.test_packed_skinny_gpu import _bits, _what, _x_dev

pytestmark = pytest.mark.gpu

COUNT, N, K = 5, 72, 300                                     # _grid_experts' shape
FIRST = (0, 3, 3, 131, 132, 390)
HOT = (0, 0, 300, 300, 300, 300)
ROUTINGS = {"surplus": FIRST, "hot": HOT, "exact-bound": (0, 129, 258, 387), "one-row": (0, 0, 0, 1, 1, 1)}
CASES = [(r, n, k) for r in ROUTINGS for n, k in ((72, 300), (200, 128))]
CASES += [("surplus", n, k) for n in (72, 200) for k in (64, 128, 192, 300) if (n, k) not in ((72, 300), (200, 128))]
SENTINEL = 0xA5
PAD = 16


def _blocks(rows):
    return sum(-(-(b - a) // 128) for a, b in zip(rows, rows[1:]))


def _slots(total_rows, count):
    return (total_rows + 127 * min(count, total_rows)) // 128


def _workspace(total_rows, count, n, k, fill=0xFF):
    """(the workspace the entry is given, the buffer it is the head of): `need` bytes of `fill` with sentinel bytes behind them."""
    need = hb.packed_linear_wide_grouped_workspace_bytes(total_rows, count, n, k)
    assert need == ((count + 1) * 4 + 15) // 16 * 16
    buf = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[:need] = fill
    return buf[:need], buf


def _tail_is_whole(buf):
    return bool((buf[-256:] == SENTINEL).all())


def _wide(pts, x, rows, bias, out_dtype, **kw):
    batch = packed.batch_of(pts)
    return hb.packed_linear_wide_grouped(x, rows if torch.is_tensor(rows) else _rows_dev(rows), batch.arena, batch.maps_dev, batch.offsets_dev,
                                         batch.bases_dev, batch.count, batch.rows, bias=bias, out_dtype=DTYPES[out_dtype], **kw)


def _block_reference(pts, x, rows, bias, out_dtype, fill=0.0):
    """The contract's right-hand side: the block kernel per group on the group's rows; rows of no group hold `fill`."""
    n = pts[0].rows
    want = torch.full((x.shape[0], n), fill, dtype=DTYPES[out_dtype], device="cuda")
    for e, pt in enumerate(pts):
        r0, r1 = rows[e], rows[e + 1]
        if r1 > r0:
            want[r0:r1] = hb.packed_linear(x[r0:r1], pt.data, pt.tables(), n, bias=None if bias is None else bias[e], out_dtype=DTYPES[out_dtype])
    return want


def _contract_holds(pts, x, bias, rows, views=True):
    total_rows, k = (int(v) for v in x.shape)
    count, n = len(pts), pts[0].rows
    for out_dtype in DTYPES:
        for b in (None, bias):
            want = _bits(_block_reference(pts, x, rows, b, out_dtype))
            ws, buf = _workspace(total_rows, count, n, k)
            for _twice in range(2):                          # the second call over what the first left in the workspace
                got = _wide(pts, x, rows, b, out_dtype, workspace=ws)
                assert tuple(got.shape) == (total_rows, n) and got.dtype == DTYPES[out_dtype]
                where = np.argwhere(_bits(got) != want)
                assert where.size == 0, (out_dtype, b is not None, where[:6])
                assert _tail_is_whole(buf)
            assert np.array_equal(_bits(_wide(pts, x, rows, b, out_dtype)), want)                # a workspace of its own
        if not views:
            continue
        # views of wider buffers: 16-byte aligned rows of X (the 16-byte loads when k % 8 == 0), an unaligned first element (element
        # by element), and Y at an odd offset into a buffer of sentinels with rows behind it
        want = _bits(_block_reference(pts, x, rows, bias, out_dtype))
        for lead, width in ((8, k + 24), (1, k + 9)):
            xw = torch.full((total_rows + PAD, width), 3.0, dtype=torch.bfloat16, device="cuda")
            xw[:total_rows, lead:lead + k] = x
            xv = xw[:total_rows, lead:lead + k]
            assert (xv.data_ptr() % 16 == 0 and xv.stride(0) % 8 == 0) == (lead == 8 and k % 8 == 0)
            yw = torch.full((total_rows + PAD, n + 9), -7.0, dtype=DTYPES[out_dtype], device="cuda")
            ws, buf = _workspace(total_rows, count, n, k)
            _wide(pts, xv, rows, bias, out_dtype, out=yw[:total_rows, 5:5 + n], workspace=ws)
            inside = yw[:total_rows, 5:5 + n].contiguous()
            assert np.array_equal(_bits(inside), np.where(_covered(rows, total_rows)[:, None], want, _bits(yw[:1, :1]))), (out_dtype, lead)
            assert bool((yw[:, :5] == -7.0).all()) and bool((yw[:, 5 + n:] == -7.0).all()) and bool((yw[total_rows:] == -7.0).all())
            assert _tail_is_whole(buf)


# ----------------------------------------------------------------------------- the bit contract

@pytest.mark.parametrize("routing,n,k", CASES)
def test_wide_grouped_is_the_block_kernel_per_group(routing, n, k):
    rows = ROUTINGS[routing]
    count, total_rows = len(rows) - 1, rows[-1]
    assert _blocks(rows) <= _slots(total_rows, count)
    if routing == "surplus":
        assert [b - a for a, b in zip(rows, rows[1:])] == [3, 0, 128, 1, 258] and (_blocks(rows), _slots(total_rows, count)) == (6, 8)
    if routing == "hot":
        assert rows[2] - rows[1] == 2 * 128 + 44
    if routing == "exact-bound":
        assert _blocks(rows) == _slots(total_rows, count) == 6
    pts, x, bias = _case(count, n, k, total_rows, 3000 + 7 * n + k)
    assert (x.data_ptr() % 16 == 0 and k % 8 == 0) == (k != 300)                                 # which X path the contiguous call takes
    _contract_holds(pts, x, bias, rows)


def test_wide_grouped_is_the_block_kernel_on_specials():
    count, total_rows = len(FIRST) - 1, FIRST[-1]
    w = np.stack([specials((N, K), seed=5100 + i) for i in range(count)])
    maps = np.stack([random_map((N, K), 5200 + i) for i in range(count)])
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")
    x = _x_dev(to_bf16_valued(gen("normal_f32", 5300, (total_rows, K)) * 8))
    bias = torch.from_numpy(gen("normal_f32", 5301, (count, N))).cuda()
    y = _wide(pts, x, FIRST, bias, "float32")
    assert not bool(torch.isfinite(y).all())                                                    # the specials reach the output
    _contract_holds(pts, x, bias, FIRST, views=False)


# ----------------------------------------------------------------------------- exact arithmetic

@functools.lru_cache(maxsize=None)
def _grid_x(total_rows):
    """Activations on the integer grid of _grid_experts for a routing of total_rows rows — made once, never written."""
    _pts, what, b, _x = _grid_experts()
    x = np.random.default_rng(6300 + total_rows).integers(-4, 5, size=(total_rows, K)).astype(np.float32)
    for i in range(COUNT):
        _grid_preconditions(x, what[i], b[i].astype(np.float64))
    x.setflags(write=False)
    return x


def test_wide_grouped_integer_grid_equals_the_float64_emulation():
    pts, what, b, _x = _grid_experts()
    total_rows = HOT[-1]
    x = _grid_x(total_rows)
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for bias_h, bias_d in ((None, None), (b, bd)):
        want = _grid_want(what, bias_h, x, HOT, total_rows)
        emu = packed.linear_grouped_wide(x, list(HOT), pts, bias=bias_h, backend="emulation")
        assert np.array_equal(emu.astype(np.float64), want)
        got = packed.linear_grouped_wide(xd, list(HOT), pts, bias=bias_d).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), np.argwhere(got != want)[:4]
        half = packed.linear_grouped_wide(xd, _rows_dev(HOT), pts, bias=bias_d, out_dtype="bfloat16")
        assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)))


def test_wide_grouped_one_hot_pins_the_decode_and_the_expert():
    s, mine, last = 3, 1, COUNT - 1
    w = np.stack([gen("normal_f32", 6820 + i, (N, K)) for i in range(COUNT)])
    maps = np.stack([random_map((N, K), 6830 + i) for i in range(COUNT)])
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")        # this test's own arena: a byte of it is flipped
    rows = [0, 0, K, K, K, 2 * K]                           # expert 1 and the last expert each see 2ˢ·I_k: groups of 300 rows, three blocks
    eye = np.eye(K, dtype=np.float32) * np.float32(2.0 ** s)
    xd = _x_dev(np.concatenate([eye, eye]))
    want = {e: (2.0 ** s) * _what(w[e], maps[e]).T for e in (mine, last)}
    for e in want:
        assert np.all(np.isfinite(want[e])) and np.array_equal(want[e].astype(np.float32).astype(np.float64), want[e])
    tiles_h, tiles_w = pts[0].map.shape
    tr, tc, r, c = tiles_h - 1, tiles_w - 1, 4, 11          # the last tile, ragged in both directions
    assert 32 * tr + r < N and 32 * tc + c < K
    at, mask = _code_byte(pts[last], tr, tc, r, c)
    for flipped in (False, True):
        if flipped:
            pts[last].data[at] ^= mask                       # a slice of the arena
        y = packed.linear_grouped_wide(xd, rows, pts).cpu().numpy().astype(np.float64)
        assert np.array_equal(y[:K], want[mine]), (flipped, np.argwhere(y[:K] != want[mine])[:4])
        bad = np.argwhere(y[K:] != want[last])
        assert [tuple(v) for v in bad] == ([(32 * tc + c, 32 * tr + r)] if flipped else []), (flipped, bad[:6])


# ----------------------------------------------------------------------------- many groups

def test_wide_grouped_many_groups_take_the_plan_past_one_entry_per_thread():
    count, n, k = 300, 32, 64
    sizes = [(0, 1, 130)[e % 3] for e in range(count)]
    rows = tuple(np.concatenate([[0], np.cumsum(sizes)]).tolist())
    total_rows = rows[-1]
    assert count > 256 and _blocks(rows) == 100 + 2 * 100 <= _slots(total_rows, count)    # two groups to a plan thread; count > 64: a bisection first
    w = np.stack([gen("heavy_f32", 7800 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), 8200 + i) for i in range(count)])           # two tiles an expert
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")
    x = _x_dev(to_bf16_valued(gen("normal_f32", 8600, (total_rows, k)) * 8))
    bias = torch.from_numpy(gen("normal_f32", 8601, (count, n))).cuda()
    rows_dev = _rows_dev(rows)
    for out_dtype in DTYPES:
        want = _bits(_block_reference(pts, x, rows, bias, out_dtype))
        ws, buf = _workspace(total_rows, count, n, k)
        got = _bits(_wide(pts, x, rows_dev, bias, out_dtype, workspace=ws))
        assert np.array_equal(got, want), (out_dtype, np.argwhere(got != want)[:6])
        assert _tail_is_whole(buf)


# ----------------------------------------------------------------------------- guards

GUARD_ROWS = (0, 130, 130, 162, 163, 300)                    # groups of 130 (two blocks), 0, 32, 1 and 137 rows: every expert but one has rows
GT = GUARD_ROWS[-1]


def _guarded(rows=GUARD_ROWS, arena=None, maps_dev=None, bases_dev=None, bias=True):
    """The entry on the integer grid over buffers with sentinels behind them → (Y of GT rows as float64, the failures of a sentinel): X
    has PAD rows of 3.0 behind it, which a missing clamp multiplies with; Y has PAD rows of −7; the workspace 256 bytes."""
    pts, _what_, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    x = _grid_x(GT)
    xbuf = torch.full((GT + PAD, K), 3.0, dtype=torch.bfloat16, device="cuda")
    xbuf[:GT] = _x_dev(x.copy())
    ybuf = torch.full((GT + PAD, N), -7.0, dtype=torch.float32, device="cuda")
    ws, wbuf = _workspace(GT, COUNT, N, K)
    hb.packed_linear_wide_grouped(xbuf[:GT], _rows_dev(rows), batch.arena if arena is None else arena,
                                  batch.maps_dev if maps_dev is None else maps_dev, batch.offsets_dev,
                                  batch.bases_dev if bases_dev is None else bases_dev, COUNT, N,
                                  bias=torch.from_numpy(b.copy()).cuda() if bias else None, out=ybuf[:GT], workspace=ws)
    got = ybuf.cpu().numpy().astype(np.float64)
    broken = [name for name, ok in (("rows of Y at or past T were written", bool(np.all(got[GT:] == -7.0))),
                                    ("bytes behind the workspace were written", _tail_is_whole(wbuf)),
                                    ("X was written", bool((xbuf[GT:] == 3.0).all()))) if not ok]
    return got[:GT], broken


def test_wide_grouped_blob_past_packed_bytes_reads_as_zeros_in_its_expert_only():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    tiles = tiles_h * tiles_w
    cut = batch.arena.numel() - 64                           # 64 bytes short of the end of the last expert's last tile
    assert cut >= COUNT * tiles * TILE_BYTES[3] and int(batch.bases[COUNT]) * 64 == batch.arena.numel()
    short = batch.arena[:cut]                                # the buffer stays whole: a kernel without the guard reads real bytes
    left = _zeroed(what, COUNT - 1, tiles_w, [tiles - 1])
    assert np.count_nonzero(left != what) > 0 and GUARD_ROWS[COUNT] > GUARD_ROWS[COUNT - 1]
    for bias in (False, True):
        got, broken = _guarded(arena=short, bias=bias)
        want = _grid_want(left, b if bias else None, _grid_x(GT), GUARD_ROWS, GT)
        assert not broken and np.array_equal(got, want), (bias, broken, np.argwhere(got != want)[:4])


def test_wide_grouped_blob_past_its_groups_own_stream_reads_as_zeros():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e = 2
    bases = batch.bases_dev.clone()
    bases[e + 1] -= 1                                        # expert 2's stream ends one unit early: its last tile does not fit
    left = _zeroed(what, e, tiles_w, [tiles_h * tiles_w - 1])
    got, broken = _guarded(bases_dev=bases)
    want = _grid_want(left, b, _grid_x(GT), GUARD_ROWS, GT)
    assert not broken, broken
    for g in (0, 1, 2, 4):                                   # expert 3 now starts a unit early: it reads bytes of the arena that mean nothing
        r0, r1 = GUARD_ROWS[g], GUARD_ROWS[g + 1]
        assert np.array_equal(got[r0:r1], want[r0:r1]), g
    assert np.array_equal(batch.bases_dev.cpu().numpy().view(np.uint64), batch.bases)            # the shared tables were not touched


def test_wide_grouped_map_codes_that_are_no_format_read_as_zeros_in_their_expert_only():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e, t_first, t_second = 4, 0 * tiles_w + 3, 1 * tiles_w + 9                                  # the second tile of step 1, the last step's
    maps = batch.maps_dev.clone()
    maps[e, t_first] = 4
    maps[e, t_second] = -1
    left = _zeroed(what, e, tiles_w, (t_first, t_second))
    got, broken = _guarded(maps_dev=maps)
    want = _grid_want(left, b, _grid_x(GT), GUARD_ROWS, GT)
    assert not broken and np.array_equal(got, want), (broken, np.argwhere(got != want)[:4])
    assert np.array_equal(batch.maps_dev.cpu().numpy().reshape(COUNT, tiles_h, tiles_w), np.stack([pt.map for pt in pts]))


# (what group_rows holds, the clamped ranges the kernels must make of it, the groups that overlap no other and keep GUARD_ROWS' range)
BAD_ROWS = {
    "decreasing": ([0, 130, 130, 162, 50, 50], [(0, 130), (130, 130), (130, 162), (162, 162), (50, 50)], (0, 2)),
    "past-T": ([0, 130, 130, 162, 163, GT + 9], [(0, 130), (130, 130), (130, 162), (162, 163), (163, GT)], (0, 2, 3, 4)),
    "negative": ([-5, 130, 130, 162, 163, GT], [(0, 130), (130, 130), (130, 162), (162, 163), (163, GT)], (0, 2, 3, 4)),
    # three clamped groups of all 300 rows: 9 blocks for 7 slots, so blocks are left out and the rows are unspecified - inside Y
    "overlapping": ([0, GT, 0, GT, 0, GT], [(0, GT), (GT, GT), (0, GT), (GT, GT), (0, GT)], ()),
}


@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_wide_grouped_group_rows_are_clamped_before_any_use(name):
    rows, clamped, right = BAD_ROWS[name]
    for e, (r0, r1) in enumerate(clamped):                  # the rule, restated
        assert r0 == min(max(rows[e], 0), GT) and r1 == min(max(rows[e + 1], r0), GT)
    if name == "overlapping":
        assert sum(-(-(r1 - r0) // 128) for r0, r1 in clamped) > _slots(GT, COUNT)
    _pts, what, b, _x = _grid_experts()
    x = _grid_x(GT)
    got, broken = _guarded(rows=rows)
    assert not broken, (name, broken)
    written = np.zeros(GT, dtype=bool)
    for e, (r0, r1) in enumerate(clamped):
        written[r0:r1] = True
        if e in right:
            assert (r0, r1) == (GUARD_ROWS[e], GUARD_ROWS[e + 1])
            want = x[r0:r1].astype(np.float64) @ what[e].T + b[e].astype(np.float64)[None, :]
            assert np.array_equal(got[r0:r1], want), (name, e)
    assert np.all(got[~written] == -7.0), (name, "a row of no clamped group was written")


def test_wide_grouped_rows_of_no_group_keep_what_out_held():
    rows, total_rows = (5, 40, 40, 170), 200
    pts, x, bias = _case(3, N, K, total_rows, 9100)
    for out_dtype in DTYPES:
        out = torch.full((total_rows, N), -7.0, dtype=DTYPES[out_dtype], device="cuda")
        got = _wide(pts, x, rows, bias, out_dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        want = _block_reference(pts, x, rows, bias, out_dtype, fill=-7.0)
        assert np.array_equal(_bits(out), _bits(want))
        assert bool((out[:5] == -7.0).all()) and bool((out[170:] == -7.0).all()) and not bool((out[5:170] == -7.0).all())


# ----------------------------------------------------------------------------- PackedExperts

def test_packed_experts_takes_the_wide_route_from_its_threshold_on(monkeypatch):
    T, small_rows = 200, [0, 1, 1, 3, 4, 5]
    rows = (0, 0, 130, 131, 200, 200)
    pts, x, bias = _case(COUNT, N, K, T, 510)
    real_entry, seen = hb.packed_linear_wide_grouped, []

    def entry(*a, **kw):
        seen.append(kw["workspace"].data_ptr())
        return real_entry(*a, **kw)

    def never(*a, **kw):
        raise AssertionError("a forward at or above the threshold left the wide entry")

    for out_dtype in DTYPES:
        for kernel in ("walk", "chunks"):
            mod = packed.PackedExperts(pts, bias=bias, out_dtype=out_dtype, kernel=kernel, wide_min_rows=64)
            today = packed.PackedExperts(pts, bias=bias, out_dtype=out_dtype, kernel=kernel)
            assert mod.backend == "hip" and mod.wide_min_rows == 64 and mod.extra_repr() == today.extra_repr() + ", wide_min_rows=64"
            kept = mod._workspace
            assert kept is not None and kept.numel() == hb.packed_linear_wide_grouped_workspace_bytes(T, COUNT, N, K)
            want = packed.linear_grouped_wide(x, list(rows), pts, bias=bias, out_dtype=out_dtype)
            assert np.array_equal(_bits(want), _bits(_block_reference(pts, x, rows, bias, out_dtype)))
            del seen[:]
            with monkeypatch.context() as mp:
                mp.setattr(hb, "packed_linear_wide_grouped", entry)
                mp.setattr(hb, "packed_linear_skinny_grouped", never)
                mp.setattr(hb, "packed_linear_skinny_grouped_chunked", never)
                for r in (_rows_dev(rows), list(rows)):
                    y = mod(x, r)
                    assert tuple(y.shape) == (T, N) and np.array_equal(_bits(y), _bits(want)), (out_dtype, kernel)
                none = mod(x, torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))          # every group empty: zeros
                assert tuple(none.shape) == (T, N) and not bool(none.any())
                assert seen == [mod._workspace.data_ptr()] * 3
            below = mod(x[:5], small_rows)                   # below the threshold: today's forward
            assert np.array_equal(_bits(below), _bits(today(x[:5], small_rows))), (out_dtype, kernel)
            assert mod._workspace.numel() >= kept.numel()    # the one kept workspace: replaced by a larger one or not at all
            again = mod(x, list(rows))                       # and the wide route on whatever the small call left there
            assert np.array_equal(_bits(again), _bits(want))
            empty = mod(x[:0], torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))         # T = 0: no launch
            assert tuple(empty.shape) == (0, N) and empty.dtype == DTYPES[out_dtype]
    zero = packed.PackedExperts(pts, bias=bias, wide_min_rows=0)
    assert tuple(zero(x[:0], [0] * (COUNT + 1)).shape) == (0, N)                                 # T = 0 on the wide route: no call either
