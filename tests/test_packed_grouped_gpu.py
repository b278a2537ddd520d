"""GPU: the grouped packed linear (packed_linear_skinny_grouped_kernel of csrc/mtq_packed.hip): every expert of one arena over its own
rows of X in one launch.

The base case is the smallest at which every index the kernel forms is exercised: count = 5 experts of n = 72 (3 tile rows, the last
ragged) × k = 300 (10 tile columns: a second ring round, the last column ragged), a different random map over all four formats per expert
(a wrong base or table row shows), group_rows = [0, 3, 3, 35, 36, 70] — groups of 3, 0, 32, 1 and 34 rows: an empty group, exactly one
chunk, a chunk loop of 32 + 2 — and 15 units per slice, which is no multiple of the 4 waves of a workgroup.

  * bit contract: for every group and every 32-row chunk of it the output is bit for bit hb.packed_linear_skinny on that chunk and that
    expert's PackedTensor at the same effective split (read back from the workspace-size function), at splits 1, 2, 0 and tiles_w + 3,
    float32 and bf16, with and without a (count, n) bias, contiguous and pitched X / Y, twice, and over a workspace of 0xFF bytes;
  * exact arithmetic: on the integer grid of tests/test_packed_gpu.py (any summation order is exact) the result EQUALS the float64
    emulation; one-hot activations pin the decode of every (n, k) position of an expert, and a flipped code byte in another expert's
    stream shows at exactly its position in that expert's rows and nowhere in this one's;
  * a long run (k = 2100: a second 64-tile chunk of map and offsets), linear_batch against the loop of packed.linear(kernel="skinny");
  * guards, which must show as wrong values and never as an access outside an allocation: packed_bytes cut short over a whole arena, a
    group's stream cut short by its own bases, map codes 4 and −1, and group_rows that decrease, pass T or start below 0, with sentinel
    rows behind X and Y;
  * PackedExperts on a kept workspace, all groups empty, and a batch rebuilt from a saved directory; a module made from a loaded list
    launches on the arena it made once, and the emulation's clamp of a device group_rows equals the kernel's, rows of no group zeros.
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
from tests.packed_cases import GRID, TILE_BYTES, _grid_preconditions, random_map
from tests.test_packed_long_k_gpu import _code_byte
from tests.test_packed_skinny_gpu import _bits, _what, _x_dev

pytestmark = pytest.mark.gpu

COUNT, N, K = 5, 72, 300
ROWS = (0, 3, 3, 35, 36, 70)
T = ROWS[-1]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def _rows_dev(rows):
    return torch.tensor(list(rows), dtype=torch.int32, device="cuda")


def _eff(total_rows, count, n, k, split):
    """The effective split, from the workspace the library asks for: split_eff · T · n floats rounded up to 16 bytes; none at 1."""
    assert 4 * total_rows * n >= 16
    need = hb.packed_linear_skinny_grouped_workspace_bytes(total_rows, count, n, k, split)
    return max(1, need // (4 * total_rows * n))


@functools.lru_cache(maxsize=None)
def _case(count, n, k, total_rows, seed):
    """(packed experts of one device arena, x bf16 device (total_rows, k), bias float32 device (count, n)) — made once, never written."""
    w = np.stack([gen("heavy_f32", seed + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), seed + 100 + i) for i in range(count)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")
    assert packed.batch_of(pts) is not None and any(not np.array_equal(maps[0], maps[i]) for i in range(1, count))
    x = _x_dev(to_bf16_valued(gen("normal_f32", seed + 200, (total_rows, k)) * 8))
    bias = torch.from_numpy(gen("normal_f32", seed + 201, (count, n))).cuda()
    return pts, x, bias


@functools.lru_cache(maxsize=None)
def _chunk_reference(key, rows, with_bias, out_dtype, eff):
    """The contract's right-hand side: hb.packed_linear_skinny per group and 32-row chunk; rows of no group are zeros."""
    pts, x, bias = _case(*key)
    n = pts[0].rows
    want = torch.zeros((x.shape[0], n), dtype=DTYPES[out_dtype], device="cuda")
    for e, pt in enumerate(pts):
        for r in range(rows[e], rows[e + 1], 32):
            c = min(32, rows[e + 1] - r)
            want[r:r + c] = hb.packed_linear_skinny(x[r:r + c], pt.data, pt.tables(), n, bias=bias[e] if with_bias else None,
                                                    out_dtype=DTYPES[out_dtype], split=eff)
    return _bits(want)


def _grouped(key, rows, with_bias, out_dtype, split, **kw):
    pts, x, bias = _case(*key)
    batch = packed.batch_of(pts)
    return hb.packed_linear_skinny_grouped(kw.pop("x", x), _rows_dev(rows), batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev,
                                           batch.count, batch.rows, bias=bias if with_bias else None, out_dtype=DTYPES[out_dtype], split=split, **kw)


def _contract_holds(key, rows, splits, out_dtype, pitched=True):
    count, n, k, total_rows, _seed = key
    pts, x, _bias = _case(*key)
    tiles_w = orc.tiles_hw(n, k)[1]
    for split in splits:
        eff = _eff(total_rows, count, n, k, split)
        assert eff == (min(split, tiles_w) if split else eff) and 1 <= eff <= tiles_w
        need = hb.packed_linear_skinny_grouped_workspace_bytes(total_rows, count, n, k, split)
        assert (need == 0) == (eff == 1)
        for with_bias in (False, True):
            want = _chunk_reference(key, rows, with_bias, out_dtype, eff)
            got = _grouped(key, rows, with_bias, out_dtype, split)
            assert tuple(got.shape) == (total_rows, n) and got.dtype == DTYPES[out_dtype]
            where = np.argwhere(_bits(got) != want)
            assert where.size == 0, (split, eff, with_bias, out_dtype, where[:6])
            assert np.array_equal(_bits(_grouped(key, rows, with_bias, out_dtype, split)), want), "two calls, the same bits"
            if need:                                 # what the workspace held before means nothing
                ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
                assert np.array_equal(_bits(_grouped(key, rows, with_bias, out_dtype, split, workspace=ws)), want), (split, with_bias)
            if pitched:                              # views of wider buffers: 16-byte aligned rows of X, an odd offset into Y
                xw = torch.full((total_rows, k + 20), 3.0, dtype=torch.bfloat16, device="cuda")
                xw[:, 8:8 + k] = x
                yw = torch.full((total_rows, n + 9), -7.0, dtype=DTYPES[out_dtype], device="cuda")
                _grouped(key, rows, with_bias, out_dtype, split, x=xw[:, 8:8 + k], out=yw[:, 5:5 + n])
                assert np.array_equal(_bits(yw[:, 5:5 + n].contiguous()), np.where(_covered(rows, total_rows)[:, None], want, _bits(yw[:1, :1])))
                assert bool((yw[:, :5] == -7.0).all()) and bool((yw[:, 5 + n:] == -7.0).all())


def _covered(rows, total_rows):
    c = np.zeros(total_rows, dtype=bool)
    for e in range(len(rows) - 1):
        c[rows[e]:rows[e + 1]] = True
    return c


# ----------------------------------------------------------------------------- the bit contract

@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_grouped_is_the_skinny_kernel_per_group_and_chunk(out_dtype):
    tiles_h, tiles_w = orc.tiles_hw(N, K)
    assert (tiles_h, tiles_w) == (3, 10) and (COUNT * tiles_h) % 4 != 0
    assert [b - a for a, b in zip(ROWS, ROWS[1:])] == [3, 0, 32, 1, 34]
    _contract_holds((COUNT, N, K, T, 500), ROWS, (1, 2, 0, tiles_w + 3), out_dtype)


@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_grouped_long_run(out_dtype):
    count, n, k, rows = 2, 40, 2100, (0, 2, 7)
    assert orc.tiles_hw(n, k)[1] == 66                       # a second 64-tile chunk of map and offsets at split 1
    assert _eff(7, count, n, k, 0) > 1
    _contract_holds((count, n, k, 7, 700), rows, (1, 0), out_dtype, pitched=False)


def test_linear_batch_is_the_loop_of_skinny_linears():
    count, m = 7, 4
    key = (count, N, K, count * m, 900)
    pts, x, bias = _case(*key)
    x3 = x.reshape(count, m, K)
    for split in (1, 0, 3):
        eff = _eff(count * m, count, N, K, split)
        for out_dtype in DTYPES:
            for b in (None, bias):
                y = packed.linear_batch(x3, pts, bias=b, out_dtype=out_dtype, split=split)
                assert tuple(y.shape) == (count, m, N)
                for e in range(count):
                    want = packed.linear(x3[e], pts[e], bias=None if b is None else b[e], out_dtype=out_dtype, kernel="skinny", split=eff)
                    assert np.array_equal(_bits(y[e].contiguous()), _bits(want)), (split, eff, out_dtype, e)


# ----------------------------------------------------------------------------- exact arithmetic

@functools.lru_cache(maxsize=None)
def _grid_experts():
    """(packed experts, Ŵ float64 (count, n, k), bias float32 (count, n), x float32 (T, k)) on the integer grid — made once, never written."""
    rng = np.random.default_rng(4242)
    w = (rng.integers(-255, 256, size=(COUNT, N, K)) * GRID).astype(np.float32)
    b = (rng.integers(-255, 256, size=(COUNT, N)) * GRID).astype(np.float32)
    x = rng.integers(-4, 5, size=(T, K)).astype(np.float32)
    maps = np.stack([random_map((N, K), 40 + i) for i in range(COUNT)])
    what = np.stack([_what(w[i], maps[i]) for i in range(COUNT)])
    for i in range(COUNT):
        _grid_preconditions(x, what[i], b[i].astype(np.float64))
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")
    for a in (what, b, x):
        a.setflags(write=False)
    return pts, what, b, x


def _grid_want(what, b, x, rows, total_rows=T):
    want = np.zeros((total_rows, N), dtype=np.float64)
    for e in range(COUNT):
        r0, r1 = rows[e], rows[e + 1]
        want[r0:r1] = x[r0:r1].astype(np.float64) @ what[e].T + (0.0 if b is None else b[e].astype(np.float64)[None, :])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return want


def test_grouped_integer_grid_equals_the_float64_emulation():
    pts, what, b, x = _grid_experts()
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for bias_h, bias_d in ((None, None), (b, bd)):
        want = _grid_want(what, bias_h, x, ROWS)
        emu = packed.linear_grouped(x, list(ROWS), pts, bias=bias_h, backend="emulation")
        assert np.array_equal(emu.astype(np.float64), want)
        for split in (1, 2, 0, 13):
            got = packed.linear_grouped(xd, list(ROWS), pts, bias=bias_d, split=split).cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (split, np.argwhere(got != want)[:4])
        half = packed.linear_grouped(xd, _rows_dev(ROWS), pts, bias=bias_d, out_dtype="bfloat16", split=0)
        assert np.array_equal(_bits(half), _bits(torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)))


def test_grouped_one_hot_pins_the_decode_and_the_expert():
    s, mine, other = 3, 1, 3
    w = np.stack([gen("normal_f32", 820 + i, (N, K)) for i in range(COUNT)])
    maps = np.stack([random_map((N, K), 830 + i) for i in range(COUNT)])
    for e in (mine, other):
        maps[e].reshape(-1)[:4] = [0, 1, 2, 3]
    pts = packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")        # this test's own arena: a byte of it is flipped
    rows = [0, 0, K, K, 2 * K, 2 * K]                       # experts 1 and 3 each see 2ˢ·I_k: groups of 300 rows, ten chunks
    eye = np.eye(K, dtype=np.float32) * np.float32(2.0 ** s)
    xd = _x_dev(np.concatenate([eye, eye]))
    want = {e: (2.0 ** s) * _what(w[e], maps[e]).T for e in (mine, other)}
    for e in want:
        assert np.all(np.isfinite(want[e])) and np.array_equal(want[e].astype(np.float32).astype(np.float64), want[e])
    tr, tc, r, c = 2, 9, 4, 11                               # ragged in both directions, of the second ring round
    assert 32 * tr + r < N and 32 * tc + c < K
    at, mask = _code_byte(pts[other], tr, tc, r, c)
    for flipped in (False, True):
        if flipped:
            pts[other].data[at] ^= mask                      # a slice of the arena
        for split in (1, 0):
            y = packed.linear_grouped(xd, rows, pts, split=split).cpu().numpy().astype(np.float64)
            assert np.array_equal(y[:K], want[mine]), (flipped, split, np.argwhere(y[:K] != want[mine])[:4])
            bad = np.argwhere(y[K:] != want[other])
            assert [tuple(v) for v in bad] == ([(32 * tc + c, 32 * tr + r)] if flipped else []), (flipped, split, bad[:6])


# ----------------------------------------------------------------------------- guards

def _zeroed(what, e, tiles_w, tiles):
    out = what.copy()
    for t in tiles:
        tr, tc = divmod(int(t), tiles_w)
        out[e, 32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = 0.0
    return out


def _guarded(pts, x, b, arena=None, maps_dev=None, bases_dev=None, rows=ROWS, split=1, x_view=None, out=None):
    batch = packed.batch_of(pts)
    return hb.packed_linear_skinny_grouped(_x_dev(x.copy()) if x_view is None else x_view, _rows_dev(rows), batch.arena if arena is None else arena,
                                           batch.maps_dev if maps_dev is None else maps_dev, batch.offsets_dev,
                                           batch.bases_dev if bases_dev is None else bases_dev, COUNT, N,
                                           bias=None if b is None else torch.from_numpy(b.copy()).cuda(), split=split, out=out)


def test_a_blob_past_packed_bytes_reads_as_zeros_in_its_expert_only():
    pts, what, b, x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    tiles = tiles_h * tiles_w
    cut = batch.arena.numel() - 64                           # 64 bytes short of the end of the last expert's last tile
    assert cut >= COUNT * tiles * TILE_BYTES[3]              # the entry refuses less
    assert int(batch.bases[COUNT]) * 64 == batch.arena.numel()
    short = batch.arena[:cut]                                # the buffer stays whole: a kernel without the guard reads real bytes
    assert short.data_ptr() == batch.arena.data_ptr() and short.numel() == cut
    left = _zeroed(what, COUNT - 1, tiles_w, [tiles - 1])
    assert np.count_nonzero(left != what) > 0
    for split in (1, 2, 0):
        for bias in (None, b):
            got = _guarded(pts, x, bias, arena=short, split=split).cpu().numpy().astype(np.float64)
            want = _grid_want(left, bias, x, ROWS)
            assert np.array_equal(got, want), (split, bias is not None, np.argwhere(got != want)[:4])


def test_a_blob_past_its_groups_own_stream_reads_as_zeros():
    pts, what, b, x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e = 2
    bases = batch.bases_dev.clone()
    bases[e + 1] -= 1                                        # expert 2's stream ends one unit early: its last tile does not fit
    left = _zeroed(what, e, tiles_w, [tiles_h * tiles_w - 1])
    for split in (1, 2):
        got = _guarded(pts, x, b, bases_dev=bases, split=split).cpu().numpy().astype(np.float64)
        want = _grid_want(left, b, x, ROWS)
        for g in (0, 1, 2, 4):                               # expert 3 now starts a unit early: it reads bytes of the arena that mean nothing
            r0, r1 = ROWS[g], ROWS[g + 1]
            assert np.array_equal(got[r0:r1], want[r0:r1]), (split, g)
    assert np.array_equal(batch.bases_dev.cpu().numpy().view(np.uint64), batch.bases)            # the shared tables were not touched


def test_map_codes_that_are_no_format_read_as_zeros_in_their_expert_only():
    pts, what, b, x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    e, t_first, t_second = 4, 0 * tiles_w + 3, 1 * tiles_w + 9                                  # ring rounds 1 and 2 of their runs at split 1
    maps = batch.maps_dev.clone()
    maps[e, t_first] = 4
    maps[e, t_second] = -1
    left = _zeroed(what, e, tiles_w, (t_first, t_second))
    for split in (1, 2, 0):
        got = _guarded(pts, x, b, maps_dev=maps, split=split).cpu().numpy().astype(np.float64)
        want = _grid_want(left, b, x, ROWS)
        assert np.array_equal(got, want), (split, np.argwhere(got != want)[:4])
    assert np.array_equal(batch.maps_dev.cpu().numpy().reshape(COUNT, tiles_h, tiles_w), np.stack([pt.map for pt in pts]))


# (what group_rows holds, the clamped ranges the kernel must make of it, the groups whose range is what ROWS gives them)
BAD_ROWS = {
    "decreasing": ([0, 3, 3, 35, 20, 20], [(0, 3), (3, 3), (3, 35), (35, 35), (20, 20)], (0, 2)),
    "past-T": ([0, 3, 3, 35, 36, T + 9], [(0, 3), (3, 3), (3, 35), (35, 36), (36, T)], (0, 2, 3, 4)),
    "negative": ([-5, 3, 3, 35, 36, T], [(0, 3), (3, 3), (3, 35), (35, 36), (36, T)], (0, 2, 3, 4)),
}


@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_group_rows_are_clamped_before_any_use(name):
    rows, clamped, right = BAD_ROWS[name]
    for e, (r0, r1) in enumerate(clamped):                  # the rule, restated
        assert r0 == min(max(rows[e], 0), T) and r1 == min(max(rows[e + 1], r0), T)
    pts, what, b, x = _grid_experts()
    pad = 16
    xbuf = torch.full((T + pad, K), 3.0, dtype=torch.bfloat16, device="cuda")                    # sentinel rows a missing clamp multiplies with
    xbuf[:T] = _x_dev(x.copy())
    for split in (1, 2):
        ybuf = torch.full((T + pad, N), -7.0, dtype=torch.float32, device="cuda")
        _guarded(pts, x, b, rows=rows, split=split, x_view=xbuf[:T], out=ybuf[:T])
        got = ybuf.cpu().numpy().astype(np.float64)
        assert np.all(got[T:] == -7.0), (name, split, "rows at or past T were written")
        written = np.zeros(T, dtype=bool)
        for e, (r0, r1) in enumerate(clamped):
            written[r0:r1] = True
            if e in right:
                assert (r0, r1) == (ROWS[e], ROWS[e + 1])
                want = x[r0:r1].astype(np.float64) @ what[e].T + b[e].astype(np.float64)[None, :]
                assert np.array_equal(got[r0:r1], want), (name, split, e)
        assert np.all(got[:T][~written] == -7.0), (name, split, "a row of no clamped group was written")
    if name == "decreasing":
        return                                               # clamped groups could overlap in general; here they do not, and rows are left
    # the emulation given the same device array applies the same rule; rows of no group are zeros on both backends
    rows_dev = _rows_dev(rows)
    emu = packed.linear_grouped(x, rows_dev, pts, bias=b, backend="emulation")
    dev = packed.linear_grouped(_x_dev(x.copy()), rows_dev, pts, bias=torch.from_numpy(b.copy()).cuda()).cpu().numpy()
    assert np.array_equal(emu, dev), name


def test_rows_of_no_group_are_zeros_on_both_backends():
    pts, what, b, x = _grid_experts()
    rows = [0, 3, 3, 35, 20, 20]                             # rows 35 .. 69 belong to no clamped group
    r0, r1 = packed.clamp_group_rows(rows, T)
    assert list(zip(r0.tolist(), r1.tolist())) == [(0, 3), (3, 3), (3, 35), (35, 35), (20, 20)]
    want = np.zeros((T, N))
    for e in (0, 2):
        want[r0[e]:r1[e]] = x[r0[e]:r1[e]].astype(np.float64) @ what[e].T + b[e].astype(np.float64)[None, :]
    rows_dev = _rows_dev(rows)
    emu = packed.linear_grouped(x, rows_dev, pts, bias=b, backend="emulation")
    assert emu.dtype == np.float32 and np.array_equal(emu.astype(np.float64), want) and not emu[35:].any()
    for split in (1, 2):
        dev = packed.linear_grouped(_x_dev(x.copy()), rows_dev, pts, bias=torch.from_numpy(b.copy()).cuda(), split=split).cpu().numpy()
        assert np.array_equal(dev.astype(np.float64), want), split


# ----------------------------------------------------------------------------- PackedExperts

def test_packed_experts_keeps_its_workspace_and_its_batch(tmp_path):
    key = (COUNT, N, K, T, 500)
    pts, x, bias = _case(*key)
    assert _eff(T, COUNT, N, K, 0) > 1 and _eff(5, COUNT, N, K, 0) > 1
    small = [0, 1, 1, 3, 4, 5]
    for out_dtype in DTYPES:
        mod = packed.PackedExperts(pts, bias=bias, out_dtype=out_dtype)
        assert mod.backend == "hip" and mod.batch is packed.batch_of(pts) and mod.bias.is_cuda
        for rows, xs in ((list(ROWS), x), (small, x[:5]), (list(ROWS), x)):   # a larger partial layout, a smaller one over it, and back
            y = mod(xs, rows)
            want = packed.linear_grouped(xs, rows, pts, bias=bias, out_dtype=out_dtype)
            assert tuple(y.shape) == (len(xs), N) and np.array_equal(_bits(y), _bits(want)), (out_dtype, len(xs))
        assert mod._workspace is not None and mod._workspace.numel() == hb.packed_linear_skinny_grouped_workspace_bytes(T, COUNT, N, K, 0)
        none = mod(x, torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))                  # every group empty: zeros
        assert tuple(none.shape) == (T, N) and not bool(none.any())
    packed.save_dir(tmp_path / "experts", {f"expert{i}": pt for i, pt in enumerate(pts)})
    loaded = list(packed.load_dir(tmp_path / "experts", device="cuda").values())
    again = packed.as_batch(loaded)
    batch = packed.batch_of(pts)
    assert again is not batch and torch.equal(again.arena, batch.arena) and np.array_equal(again.bases, batch.bases)
    assert torch.equal(again.maps_dev, batch.maps_dev) and torch.equal(again.offsets_dev, batch.offsets_dev) and torch.equal(again.bases_dev, batch.bases_dev)
    mod2 = packed.PackedExperts(loaded, bias=bias)
    assert np.array_equal(_bits(mod2(x, list(ROWS))), _bits(packed.PackedExperts(pts, bias=bias)(x, list(ROWS))))


def test_packed_experts_multiplies_with_the_batch_it_made(tmp_path, monkeypatch):
    """A list that is no pack_batch batch (a loaded directory) is concatenated once, in the constructor: forward launches on that arena and
    never builds another.  linear_batch resolves its list once."""
    key = (COUNT, N, K, T, 500)
    pts, x, bias = _case(*key)
    packed.save_dir(tmp_path / "experts", {f"expert{i}": pt for i, pt in enumerate(pts)})
    loaded = list(packed.load_dir(tmp_path / "experts", device="cuda").values())
    assert packed.batch_of(loaded) is None
    mod = packed.PackedExperts(loaded, bias=bias, out_dtype="bfloat16")
    assert mod.backend == "hip" and mod.batch.arena.is_cuda and not hasattr(mod, "_pts")
    want = packed.linear_grouped(x, list(ROWS), pts, bias=bias, out_dtype="bfloat16")
    real_as_batch, real_entry, seen, made = packed.as_batch, hb.packed_linear_skinny_grouped, [], []

    def no_as_batch(*a, **kw):
        raise AssertionError("as_batch ran inside forward")

    def entry(x_, rows_, arena, maps_dev, offsets_dev, bases_dev, *a, **kw):
        seen.append((arena.data_ptr(), maps_dev.data_ptr(), offsets_dev.data_ptr(), bases_dev.data_ptr()))
        return real_entry(x_, rows_, arena, maps_dev, offsets_dev, bases_dev, *a, **kw)

    monkeypatch.setattr(hb, "packed_linear_skinny_grouped", entry)
    monkeypatch.setattr(packed, "as_batch", no_as_batch)
    rows_dev = _rows_dev(ROWS)
    for rows in (list(ROWS), rows_dev, rows_dev):
        assert np.array_equal(_bits(mod(x, rows)), _bits(want))
    own = (mod.batch.arena.data_ptr(), mod.batch.maps_dev.data_ptr(), mod.batch.offsets_dev.data_ptr(), mod.batch.bases_dev.data_ptr())
    assert seen == [own] * 3
    # a PackedBatch handed to linear_grouped / linear_batch is taken as it is
    assert np.array_equal(_bits(packed.linear_grouped(x, rows_dev, mod.batch, bias=bias, out_dtype="bfloat16")), _bits(want))

    def counting(*a, **kw):
        made.append(1)
        return real_as_batch(*a, **kw)

    monkeypatch.setattr(packed, "as_batch", counting)
    x3 = x[:COUNT * 4].reshape(COUNT, 4, K)
    y3 = packed.linear_batch(x3, loaded, split=1)
    assert made == [1], "linear_batch concatenates a loaded list once"
    assert np.array_equal(_bits(y3), _bits(packed.linear_batch(x3, pts, split=1)))
