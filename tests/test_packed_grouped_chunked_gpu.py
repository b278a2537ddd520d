"""GPU: the chunked grouped packed linear (packed_grouped_plan_kernel + packed_linear_skinny_grouped_chunked_kernel of
csrc/mtq_packed.hip): a wave per (K slice, 32-row chunk of a group, tile row), the chunk list made from group_rows on the device.

The oracle for bits is never the new code: the walking entry (hb.packed_linear_skinny_grouped), the per-chunk
packed.linear(kernel="skinny"), and on the integer grid the float64 emulation.

The base shape is tests/test_packed_grouped_gpu.py's: count = 5 experts of n = 72 × k = 300 (3 tile rows × 10 tile columns, both
ragged), a different random map per expert.  The routings:

  (0, 3, 3, 35, 36, 70)        T = 70   that file's case: 5 chunks in 7 slots
  (0, 0, 130, 131, 200, 200)   T = 200  a hot group of 4 × 32 + 2 rows, empty groups first and last, 9 chunks in 11 slots: surplus waves
  (0, 33, 66, 99), count 3     T = 99   6 chunks in 6 slots: the bound met exactly, every slot used
  (0, 0, 0, 1, 1, 1)           T = 1    one row, one chunk, one slot

  * for each, float32 and bf16, the result is the walking entry's bit for bit at splits 1, 2, 0 and tiles_w + 3, with and without bias,
    with pitched X and Y, called twice over a workspace of 0xFF bytes; the hot routing also chunk by chunk against
    packed.linear(kernel="skinny") at the effective split;
  * the integer grid EQUALS the float64 emulation on the hot routing; k = 2100 reaches a second 64-tile hand-out; count = 300 with
    groups of 0, 1 and 40 rows takes the plan kernel past one entry per thread and the group search past one window of 64;
  * guards over buffers that stay whole, with sentinel rows behind X, Y and the workspace: packed_bytes cut short, a group's stream cut
    short by its own bases, map codes 4 and −1, and group_rows that decrease, overlap, end at T + 9 or start below 0;
  * PackedExperts(kernel="chunks") on its kept workspace and on the arena its constructor made; linear_batch(kernel="chunks").
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
from tests.packed_cases import TILE_BYTES, _grid_preconditions, random_map
from tests.test_packed_grouped_gpu import COUNT, DTYPES, K, N, _case, _covered, _eff, _grid_experts, _grid_want, _rows_dev, _zeroed
from tests.test_packed_skinny_gpu import _bits, _x_dev

pytestmark = pytest.mark.gpu

HOT = (0, 0, 130, 131, 200, 200)
ROUTINGS = {
    "base": ((COUNT, N, K, 70, 500), (0, 3, 3, 35, 36, 70)),
    "hot": ((COUNT, N, K, 200, 510), HOT),
    "exact-bound": ((3, N, K, 99, 520), (0, 33, 66, 99)),
    "one-row": ((COUNT, N, K, 1, 530), (0, 0, 0, 1, 1, 1)),
}
SENTINEL = 0xA5


def _chunk_count(rows):
    return sum(-(-(b - a) // 32) for a, b in zip(rows, rows[1:]))


def _slots(total_rows, count):
    return (total_rows + 31 * min(count, total_rows)) // 32


def _workspace(total_rows, count, n, k, split, fill=0xFF):
    """(the workspace the entry is given, the buffer it is the head of): `need` bytes of `fill` with sentinel bytes behind them."""
    need = hb.packed_linear_skinny_grouped_chunked_workspace_bytes(total_rows, count, n, k, split)
    plan = ((count + 1) * 4 + 15) // 16 * 16
    assert need == plan + hb.packed_linear_skinny_grouped_workspace_bytes(total_rows, count, n, k, split) and need > 0
    buf = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[:need] = fill
    return buf[:need], buf


def _tail_is_whole(buf):
    return bool((buf[-256:] == SENTINEL).all())


def _entry(which, key, rows, with_bias, out_dtype, split, **kw):
    pts, x, bias = _case(*key)
    batch = packed.batch_of(pts)
    fn = hb.packed_linear_skinny_grouped if which == "walk" else hb.packed_linear_skinny_grouped_chunked
    return fn(kw.pop("x", x), _rows_dev(rows), batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, batch.count, batch.rows,
              bias=bias if with_bias else None, out_dtype=DTYPES[out_dtype], split=split, **kw)


# ----------------------------------------------------------------------------- the bit contract

@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_chunked_is_the_walking_entry_bit_for_bit(routing, out_dtype):
    key, rows = ROUTINGS[routing]
    count, n, k, total_rows, _seed = key
    pts, x, _bias = _case(*key)
    tiles_w = orc.tiles_hw(n, k)[1]
    assert len(rows) == count + 1 and rows[-1] == total_rows and _chunk_count(rows) <= _slots(total_rows, count)
    if routing == "hot":
        assert (_chunk_count(rows), _slots(total_rows, count)) == (9, 11)
    if routing == "exact-bound":
        assert _chunk_count(rows) == _slots(total_rows, count) == 6
    for split in (1, 2, 0, tiles_w + 3):
        for with_bias in (False, True):
            want = _bits(_entry("walk", key, rows, with_bias, out_dtype, split))
            for _twice in range(2):
                ws, buf = _workspace(total_rows, count, n, k, split)
                got = _entry("chunks", key, rows, with_bias, out_dtype, split, workspace=ws)
                assert tuple(got.shape) == (total_rows, n) and got.dtype == DTYPES[out_dtype]
                where = np.argwhere(_bits(got) != want)
                assert where.size == 0, (routing, split, with_bias, where[:6])
                assert _tail_is_whole(buf)
            assert np.array_equal(_bits(_entry("chunks", key, rows, with_bias, out_dtype, split)), want)    # a workspace of its own
            # views of wider buffers: 16-byte aligned rows of X, an odd offset into Y
            xw = torch.full((total_rows, k + 20), 3.0, dtype=torch.bfloat16, device="cuda")
            xw[:, 8:8 + k] = x
            yw = torch.full((total_rows, n + 9), -7.0, dtype=DTYPES[out_dtype], device="cuda")
            _entry("chunks", key, rows, with_bias, out_dtype, split, x=xw[:, 8:8 + k], out=yw[:, 5:5 + n])
            assert np.array_equal(_bits(yw[:, 5:5 + n].contiguous()), np.where(_covered(rows, total_rows)[:, None], want, _bits(yw[:1, :1])))
            assert bool((yw[:, :5] == -7.0).all()) and bool((yw[:, 5 + n:] == -7.0).all())


@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_chunked_is_the_skinny_linear_chunk_by_chunk(out_dtype):
    key, rows = ROUTINGS["hot"]
    count, n, k, total_rows, _seed = key
    pts, x, bias = _case(*key)
    for split in (1, 0, 3):
        eff = _eff(total_rows, count, n, k, split)
        for b in (None, bias):
            y = packed.linear_grouped(x, _rows_dev(rows), pts, bias=b, out_dtype=out_dtype, split=split, kernel="chunks")
            for e in range(count):
                for r in range(rows[e], rows[e + 1], 32):
                    c = min(32, rows[e + 1] - r)
                    want = packed.linear(x[r:r + c], pts[e], bias=None if b is None else b[e], out_dtype=out_dtype, kernel="skinny", split=eff)
                    assert np.array_equal(_bits(y[r:r + c].contiguous()), _bits(want)), (split, eff, e, r)
            assert not bool(y[~torch.from_numpy(_covered(rows, total_rows)).cuda()].any())


@functools.lru_cache(maxsize=None)
def _grid_x(total_rows):
    """Activations on the integer grid of _grid_experts for a routing of total_rows rows — made once, never written."""
    _pts, what, b, _x = _grid_experts()
    x = np.random.default_rng(4300 + total_rows).integers(-4, 5, size=(total_rows, K)).astype(np.float32)
    for i in range(COUNT):
        _grid_preconditions(x, what[i], b[i].astype(np.float64))
    x.setflags(write=False)
    return x


def test_chunked_integer_grid_equals_the_float64_emulation():
    pts, what, b, _x = _grid_experts()
    total_rows = HOT[-1]
    x = _grid_x(total_rows)
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for bias_h, bias_d in ((None, None), (b, bd)):
        want = _grid_want(what, bias_h, x, HOT, total_rows)
        emu = packed.linear_grouped(x, list(HOT), pts, bias=bias_h, backend="emulation", kernel="chunks")
        assert np.array_equal(emu.astype(np.float64), want)
        for split in (1, 2, 0, 13):
            got = packed.linear_grouped(xd, list(HOT), pts, bias=bias_d, split=split, kernel="chunks").cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (split, np.argwhere(got != want)[:4])
        half = packed.linear_grouped(xd, _rows_dev(HOT), pts, bias=bias_d, out_dtype="bfloat16", split=0, kernel="chunks")
        assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)))


def test_chunked_long_run():
    count, n, k, rows = 2, 40, 2100, (0, 35, 40)             # chunks of 32 + 3 and of 5 rows
    assert orc.tiles_hw(n, k)[1] == 66                       # a second 64-tile hand-out of map and offsets at split 1
    key = (count, n, k, rows[-1], 700)
    assert _eff(rows[-1], count, n, k, 0) > 1
    for out_dtype in DTYPES:
        for split in (1, 0):
            for with_bias in (False, True):
                want = _bits(_entry("walk", key, rows, with_bias, out_dtype, split))
                assert np.array_equal(_bits(_entry("chunks", key, rows, with_bias, out_dtype, split)), want), (out_dtype, split, with_bias)


def test_chunked_many_groups_take_the_plan_past_one_entry_per_thread():
    count, n, k = 300, 32, 64
    sizes = [(0, 1, 40)[(e * 7 + e // 3) % 3] for e in range(count)]
    assert {sizes.count(v) > 50 for v in (0, 1, 40)} == {True} and count > 256
    rows = tuple(np.concatenate([[0], np.cumsum(sizes)]).tolist())
    total_rows = rows[-1]
    assert _chunk_count(rows) == sizes.count(1) + 2 * sizes.count(40) <= _slots(total_rows, count)
    w = np.stack([gen("heavy_f32", 800 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), 1200 + i) for i in range(count)])           # two tiles an expert
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")
    batch = packed.batch_of(pts)
    x = _x_dev(to_bf16_valued(gen("normal_f32", 1600, (total_rows, k)) * 8))
    bias = torch.from_numpy(gen("normal_f32", 1601, (count, n))).cuda()
    rows_dev = _rows_dev(rows)

    def run(fn, out_dtype, split, **kw):
        return fn(x, rows_dev, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n, bias=bias, out_dtype=DTYPES[out_dtype],
                  split=split, **kw)

    for out_dtype in DTYPES:
        for split in (1, 2, 0):
            want = _bits(run(hb.packed_linear_skinny_grouped, out_dtype, split))
            ws, buf = _workspace(total_rows, count, n, k, split)
            got = _bits(run(hb.packed_linear_skinny_grouped_chunked, out_dtype, split, workspace=ws))
            assert np.array_equal(got, want), (out_dtype, split, np.argwhere(got != want)[:6])
            assert _tail_is_whole(buf)
    # and the walking entry's own oracle on a few groups of each size, some past the 256th among them
    y = run(hb.packed_linear_skinny_grouped_chunked, "float32", 1)
    for e in (0, 1, 2, 3, 4, 5, 255, 256, 257, 297, 298, 299):
        for r in range(rows[e], rows[e + 1], 32):
            c = min(32, rows[e + 1] - r)
            want = packed.linear(x[r:r + c], pts[e], bias=bias[e], kernel="skinny", split=1)
            assert np.array_equal(_bits(y[r:r + c].contiguous()), _bits(want)), (e, r)


def test_linear_batch_with_chunks_is_the_loop_of_skinny_linears():
    count, m = 7, 4
    key = (count, N, K, count * m, 900)
    pts, x, bias = _case(*key)
    x3 = x.reshape(count, m, K)
    for split in (1, 0, 3):
        eff = _eff(count * m, count, N, K, split)
        for out_dtype in DTYPES:
            for b in (None, bias):
                y = packed.linear_batch(x3, pts, bias=b, out_dtype=out_dtype, split=split, kernel="chunks")
                assert tuple(y.shape) == (count, m, N)
                for e in range(count):
                    want = packed.linear(x3[e], pts[e], bias=None if b is None else b[e], out_dtype=out_dtype, kernel="skinny", split=eff)
                    assert np.array_equal(_bits(y[e].contiguous()), _bits(want)), (split, eff, out_dtype, e)


# ----------------------------------------------------------------------------- guards

GUARD_ROWS = (0, 66, 66, 98, 99, 140)                        # groups of 66 (three chunks), 0, 32, 1 and 41 rows: every expert but one has rows
GT = GUARD_ROWS[-1]
PAD = 16


def _guarded(rows=GUARD_ROWS, split=1, arena=None, maps_dev=None, bases_dev=None, bias=True):
    """The chunked entry on the integer grid over buffers with sentinels behind them → (Y of GT rows as float64, the failures of a
    sentinel): X has PAD rows of 3.0 behind it, which a missing clamp multiplies with; Y has PAD rows of −7; the workspace 256 bytes."""
    pts, _what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    x = _grid_x(GT)
    xbuf = torch.full((GT + PAD, K), 3.0, dtype=torch.bfloat16, device="cuda")
    xbuf[:GT] = _x_dev(x.copy())
    ybuf = torch.full((GT + PAD, N), -7.0, dtype=torch.float32, device="cuda")
    ws, wbuf = _workspace(GT, COUNT, N, K, split)
    hb.packed_linear_skinny_grouped_chunked(xbuf[:GT], _rows_dev(rows), batch.arena if arena is None else arena,
                                            batch.maps_dev if maps_dev is None else maps_dev, batch.offsets_dev,
                                            batch.bases_dev if bases_dev is None else bases_dev, COUNT, N,
                                            bias=torch.from_numpy(b.copy()).cuda() if bias else None, split=split, out=ybuf[:GT], workspace=ws)
    got = ybuf.cpu().numpy().astype(np.float64)
    broken = [name for name, ok in (("rows of Y at or past T were written", bool(np.all(got[GT:] == -7.0))),
                                    ("bytes behind the workspace were written", _tail_is_whole(wbuf)),
                                    ("X was written", bool((xbuf[GT:] == 3.0).all()))) if not ok]
    return got[:GT], broken


def test_chunked_blob_past_packed_bytes_reads_as_zeros_in_its_expert_only():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    tiles = tiles_h * tiles_w
    cut = batch.arena.numel() - 64                           # 64 bytes short of the end of the last expert's last tile
    assert cut >= COUNT * tiles * TILE_BYTES[3] and int(batch.bases[COUNT]) * 64 == batch.arena.numel()
    short = batch.arena[:cut]                                # the buffer stays whole: a kernel without the guard reads real bytes
    left = _zeroed(what, COUNT - 1, tiles_w, [tiles - 1])
    assert np.count_nonzero(left != what) > 0 and GUARD_ROWS[COUNT] > GUARD_ROWS[COUNT - 1]
    for split in (1, 2, 0):
        for bias in (False, True):
            got, broken = _guarded(split=split, arena=short, bias=bias)
            want = _grid_want(left, b if bias else None, _grid_x(GT), GUARD_ROWS, GT)
            assert not broken and np.array_equal(got, want), (split, bias, broken, np.argwhere(got != want)[:4])


def test_chunked_blob_past_its_groups_own_stream_reads_as_zeros():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e = 2
    bases = batch.bases_dev.clone()
    bases[e + 1] -= 1                                        # expert 2's stream ends one unit early: its last tile does not fit
    left = _zeroed(what, e, tiles_w, [tiles_h * tiles_w - 1])
    for split in (1, 2):
        got, broken = _guarded(split=split, bases_dev=bases)
        want = _grid_want(left, b, _grid_x(GT), GUARD_ROWS, GT)
        assert not broken, broken
        for g in (0, 1, 2, 4):                               # expert 3 now starts a unit early: it reads bytes of the arena that mean nothing
            r0, r1 = GUARD_ROWS[g], GUARD_ROWS[g + 1]
            assert np.array_equal(got[r0:r1], want[r0:r1]), (split, g)
    assert np.array_equal(batch.bases_dev.cpu().numpy().view(np.uint64), batch.bases)            # the shared tables were not touched


def test_chunked_map_codes_that_are_no_format_read_as_zeros_in_their_expert_only():
    pts, what, b, _x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e, t_first, t_second = 4, 0 * tiles_w + 3, 1 * tiles_w + 9                                  # ring rounds 1 and 2 of their runs at split 1
    maps = batch.maps_dev.clone()
    maps[e, t_first] = 4
    maps[e, t_second] = -1
    left = _zeroed(what, e, tiles_w, (t_first, t_second))
    for split in (1, 2, 0):
        got, broken = _guarded(split=split, maps_dev=maps)
        want = _grid_want(left, b, _grid_x(GT), GUARD_ROWS, GT)
        assert not broken and np.array_equal(got, want), (split, broken, np.argwhere(got != want)[:4])
    assert np.array_equal(batch.maps_dev.cpu().numpy().reshape(COUNT, tiles_h, tiles_w), np.stack([pt.map for pt in pts]))


# (what group_rows holds, the clamped ranges the kernels must make of it, the groups that overlap no other and keep GUARD_ROWS' range)
BAD_ROWS = {
    "decreasing": ([0, 66, 66, 98, 50, 50], [(0, 66), (66, 66), (66, 98), (98, 98), (50, 50)], (0, 2)),
    "past-T": ([0, 66, 66, 98, 99, GT + 9], [(0, 66), (66, 66), (66, 98), (98, 99), (99, GT)], (0, 2, 3, 4)),
    "negative": ([-5, 66, 66, 98, 99, GT], [(0, 66), (66, 66), (66, 98), (98, 99), (99, GT)], (0, 2, 3, 4)),
    # three clamped groups of all 140 rows: 15 chunks for 9 slots, so chunks are left out and the rows are unspecified - inside Y
    "overlapping": ([0, GT, 0, GT, 0, GT], [(0, GT), (GT, GT), (0, GT), (GT, GT), (0, GT)], ()),
}


@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_chunked_group_rows_are_clamped_before_any_use(name):
    rows, clamped, right = BAD_ROWS[name]
    for e, (r0, r1) in enumerate(clamped):                  # the rule, restated
        assert r0 == min(max(rows[e], 0), GT) and r1 == min(max(rows[e + 1], r0), GT)
    if name == "overlapping":
        assert sum(-(-(r1 - r0) // 32) for r0, r1 in clamped) > _slots(GT, COUNT)
    _pts, what, b, _x = _grid_experts()
    x = _grid_x(GT)
    for split in (1, 2):
        got, broken = _guarded(rows=rows, split=split)
        assert not broken, (name, split, broken)
        written = np.zeros(GT, dtype=bool)
        for e, (r0, r1) in enumerate(clamped):
            written[r0:r1] = True
            if e in right:
                assert (r0, r1) == (GUARD_ROWS[e], GUARD_ROWS[e + 1])
                want = x[r0:r1].astype(np.float64) @ what[e].T + b[e].astype(np.float64)[None, :]
                assert np.array_equal(got[r0:r1], want), (name, split, e)
        assert np.all(got[~written] == -7.0), (name, split, "a row of no clamped group was written")


# ----------------------------------------------------------------------------- PackedExperts

def test_packed_experts_with_chunks_keeps_its_workspace_and_launches_on_its_arena(tmp_path, monkeypatch):
    key, rows = ROUTINGS["hot"]
    pts, x, bias = _case(*key)
    T = rows[-1]
    small = [0, 1, 1, 3, 4, 5]
    packed.save_dir(tmp_path / "experts", {f"expert{i}": pt for i, pt in enumerate(pts)})
    loaded = list(packed.load_dir(tmp_path / "experts", device="cuda").values())
    assert packed.batch_of(loaded) is None
    want = {out_dtype: (packed.linear_grouped(x, list(rows), pts, bias=bias, out_dtype=out_dtype),
                        packed.linear_grouped(x[:5], small, pts, bias=bias, out_dtype=out_dtype)) for out_dtype in DTYPES}     # the walking entry's
    real_entry, seen = hb.packed_linear_skinny_grouped_chunked, []

    def entry(x_, rows_, arena, maps_dev, offsets_dev, bases_dev, *a, **kw):
        seen.append((arena.data_ptr(), maps_dev.data_ptr(), offsets_dev.data_ptr(), bases_dev.data_ptr(), kw["workspace"].data_ptr()))
        return real_entry(x_, rows_, arena, maps_dev, offsets_dev, bases_dev, *a, **kw)

    def never(*a, **kw):
        raise AssertionError("forward left the module's kernel or its batch")

    for out_dtype in DTYPES:
        mod = packed.PackedExperts(loaded, bias=bias, out_dtype=out_dtype, kernel="chunks")
        assert mod.backend == "hip" and mod.kernel == "chunks" and mod.batch.arena.is_cuda
        with monkeypatch.context() as mp:
            mp.setattr(hb, "packed_linear_skinny_grouped_chunked", entry)
            mp.setattr(hb, "packed_linear_skinny_grouped", never)
            mp.setattr(packed, "as_batch", never)
            del seen[:]
            rows_dev = _rows_dev(rows)
            for r, xs, w in ((rows_dev, x, want[out_dtype][0]), (small, x[:5], want[out_dtype][1]), (list(rows), x, want[out_dtype][0])):
                y = mod(xs, r)
                assert tuple(y.shape) == (len(xs), N) and np.array_equal(_bits(y), _bits(w)), (out_dtype, len(xs))
            need = hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, COUNT, N, K, 0)
            assert mod._workspace is not None and mod._workspace.numel() == need
            own = (mod.batch.arena.data_ptr(), mod.batch.maps_dev.data_ptr(), mod.batch.offsets_dev.data_ptr(), mod.batch.bases_dev.data_ptr(),
                   mod._workspace.data_ptr())
            assert seen == [own] * 3                         # the constructor's arena, one kept workspace
            none = mod(x, torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))              # every group empty: zeros
            assert tuple(none.shape) == (T, N) and not bool(none.any())
            empty = mod(x[:0], torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))         # T = 0: no launch
            assert tuple(empty.shape) == (0, N) and len(seen) == 4
    # at split 1 the walking entry keeps no workspace; the chunked one keeps its plan
    mod1 = packed.PackedExperts(pts, bias=bias, split=1, kernel="chunks")
    assert np.array_equal(_bits(mod1(x, list(rows))), _bits(packed.linear_grouped(x, list(rows), pts, bias=bias, split=1)))
    assert mod1._workspace is not None and mod1._workspace.numel() == ((COUNT + 1) * 4 + 15) // 16 * 16
    assert mod1.batch is packed.batch_of(pts)
