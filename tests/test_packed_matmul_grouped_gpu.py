"""GPU: the grouped skinny matmul for (k, n) experts - packed_matmul_skinny_grouped_kernel ("walk") and
packed_matmul_skinny_grouped_chunked_kernel ("chunks") of csrc/mtq_packed.hip - and what packed.py builds on them.

Base: count = 5 experts with k = 300, n = 72, a different random map per expert over the (k, n) grid (10 x 3 tiles, both ragged); n = 72
gives three units to a four-wave workgroup, so one wave exits at the seam.  Routings:
  (0, 3, 3, 35, 36, 70)          groups of 3, 0, 32, 1 and 34 rows: an empty group, exactly one chunk, a chunk loop of 32 + 2;
  (0, 0, 130, 131, 200, 200)     a hot group of 4 x 32 + 2 rows, empty groups first and last, surplus chunk slots;
  (0, 33, 66, 99), count = 3     the slot bound met exactly;
  (0, 0, 0, 1, 1, 1)             one row.

  * bits, on the words: walk == chunks == matmul(kernel="skinny") per 32-row chunk at the effective split ==
    linear_grouped(kernel="walk") on the arena of all-bf16 packings of unpack(P̂[e])ᵀ at the same split; float32 and bf16, with and
    without bias, splits 0, 1, 2, tiles_kh + 3; X contiguous and an odd-pitch unaligned view, Y into sentinels, twice over a workspace
    of 0xFF bytes with sentinel bytes behind it; the specials weight (NaN-aware); other shapes on the first routing;
  * exact arithmetic, independent of every other kernel: the integer grid EQUALS the float64 product, one-hot rows return P̂[e], a
    flipped code byte changes exactly its output;
  * count = 300: the plan past one entry per thread, the search past one window;
  * guards over buffers that stay whole; the module and batch forms.
The oracle for bits is never the new code."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import GRID, TILE_BYTES, _grid_preconditions, random_map, specials, uniform_map
from tests.test_packed_grouped_gpu import _covered, _rows_dev
from tests.test_packed_long_k_gpu import _code_byte
from tests.test_packed_matmul_skinny_gpu import _bits, _phat, _same, _x_dev

pytestmark = pytest.mark.gpu

COUNT, N, K = 5, 72, 300
ROUTINGS = {"mixed": (0, 3, 3, 35, 36, 70), "hot": (0, 0, 130, 131, 200, 200), "exact-bound": (0, 33, 66, 99), "one-row": (0, 0, 0, 1, 1, 1)}
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
ENTRIES = {"walk": (hb.packed_matmul_skinny_grouped, hb.packed_matmul_skinny_grouped_workspace_bytes),
           "chunks": (hb.packed_matmul_skinny_grouped_chunked, hb.packed_matmul_skinny_grouped_chunked_workspace_bytes)}


def _eff(T, count, n, k, split):
    """The effective split, from the grouped LINEAR entry's size function (the contract says the two agree; the host tests hold them to it)."""
    assert 4 * T * n >= 16
    need = hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, split)
    return max(1, need // (4 * T * n))


@functools.lru_cache(maxsize=None)
def _case(count, n, k, T, seed, kind="heavy"):
    """(the (k, n) experts of one device arena, the arena of all-bf16 row-layout packings of unpack(P̂[e])ᵀ, x contiguous, x as an odd-pitch
    unaligned view, bias) - made once, never written."""
    w = np.stack([specials((n, k), seed=seed + i) if kind == "specials" else gen("heavy_f32", seed + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((k, n), seed + 100 + i) for i in range(count)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")
    batch = packed.batch_of(pts)
    assert batch is not None and (batch.rows, batch.cols) == (k, n) and (count == 1 or any(not np.array_equal(maps[0], m) for m in maps[1:]))
    back = packed.unpack_batch_transposed(pts, backend="hip", dtype="bfloat16")                  # (count, n, k): unpack(P̂[e])ᵀ
    ref = packed.pack_batch(back, np.stack([uniform_map((n, k), 0)] * count), backend="hip")
    x = _x_dev(to_bf16_valued(gen("normal_f32", seed + 200, (T, k)) * 8))
    wide = torch.zeros((T, k + 9), dtype=torch.bfloat16, device="cuda")
    wide[:, 1:1 + k] = x
    view = wide[:, 1:1 + k]
    assert view.data_ptr() % 16 != 0 and view.stride(0) % 8 != 0
    return pts, ref, x, view, torch.from_numpy(gen("normal_f32", seed + 201, (count, n))).cuda()


def _call(kernel, pts, x, rows, bias, dtype, split, **kw):
    batch = packed.batch_of(pts)
    return ENTRIES[kernel][0](x, rows if torch.is_tensor(rows) else _rows_dev(rows), batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev,
                              batch.count, batch.cols, bias=bias, out_dtype=dtype, split=split, **kw)


def _chunk_reference(pts, x, rows, bias, dtype, eff):
    """The contract's right-hand side: hb.packed_matmul_skinny per group and 32-row chunk; rows of no group are zeros."""
    n = pts[0].cols
    want = torch.zeros((x.shape[0], n), dtype=dtype, device="cuda")
    for e, pt in enumerate(pts):
        for r in range(rows[e], rows[e + 1], 32):
            c = min(32, rows[e + 1] - r)
            want[r:r + c] = hb.packed_matmul_skinny(x[r:r + c], pt.data, pt.tables(), n, bias=None if bias is None else bias[e], out_dtype=dtype,
                                                    split=eff)
    return want


def _contract_holds(count, n, k, rows, seed, out_dtype, splits, kind="heavy", views=True):
    T = rows[-1]
    pts, ref, x, view, bias_d = _case(count, n, k, T, seed, kind)
    dtype, nan = DTYPES[out_dtype], kind == "specials"
    cover = torch.from_numpy(_covered(rows, T)).cuda()
    for split in splits:
        eff = _eff(T, count, n, k, split)
        assert 1 <= eff <= -(-k // 32) and (split == 0 or eff == min(split, -(-k // 32)))
        for bias in (None, bias_d):
            what = (count, n, k, rows, out_dtype, split, eff, bias is not None)
            want = _chunk_reference(pts, x, rows, bias, dtype, eff)
            lin = packed.linear_grouped(x, _rows_dev(rows), ref, bias=bias, out_dtype=out_dtype, split=split, kernel="walk")
            _same(lin, want, nan, what + ("the linear walk on the transposed arena",))
            for kernel, (_fn, size) in ENTRIES.items():
                need = size(T, count, n, k, split)
                assert (kernel == "chunks" and need > 0) or (need == 0) == (eff == 1)
                ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
                for xd in ((x, view) if views else (x,)):
                    got = _call(kernel, pts, xd, rows, bias, dtype, split, workspace=ws[:need] if need else None)
                    assert tuple(got.shape) == (T, n) and got.dtype == dtype
                    _same(got, want, nan, what + (kernel, xd is view))
                again = _call(kernel, pts, x, rows, bias, dtype, split, workspace=ws[:need] if need else None)
                _same(again, want, nan, what + (kernel, "again"))
                assert bool((ws[need:] == 0xFF).all()), what + (kernel, "bytes behind the workspace")
                if views:                                # Y into a pitched buffer of sentinels: rows of no group and everything around stay
                    yw = torch.full((T + 2, n + 9), -7.0, dtype=dtype, device="cuda")
                    out = yw[1:1 + T, 5:5 + n]
                    _call(kernel, pts, view, rows, bias, dtype, split, out=out)
                    _same(out.contiguous(), torch.where(cover[:, None], want, torch.full_like(want, -7.0)), nan, what + (kernel, "pitched y"))
                    yw[1:1 + T, 5:5 + n] = -7.0
                    assert bool((yw == -7.0).all()), what + (kernel, "around y")


@pytest.mark.parametrize("out_dtype", list(DTYPES))
@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_walk_and_chunks_are_the_skinny_matmul_per_chunk_and_the_linear_walk_bit_for_bit(routing, out_dtype):
    rows = ROUTINGS[routing]
    count = len(rows) - 1
    tiles_kh, tiles_nw = -(-K // 32), -(-N // 32)
    assert (tiles_kh, tiles_nw) == (10, 3) and (count * tiles_nw) % 4 != 0
    if routing == "exact-bound":
        assert sum(-(-(b - a) // 32) for a, b in zip(rows, rows[1:])) == (rows[-1] + 31 * min(count, rows[-1])) // 32 == 6
    _contract_holds(count, N, K, rows, 500, out_dtype, (0, 1, 2, tiles_kh + 3))


@pytest.mark.parametrize("out_dtype", list(DTYPES))
def test_the_specials_weight_bit_for_bit(out_dtype):
    _contract_holds(COUNT, N, K, ROUTINGS["mixed"], 900, out_dtype, (0, 1, 2), kind="specials")


@pytest.mark.parametrize("n,k", [(40, 100), (200, 104)])
def test_other_shapes_bit_for_bit(n, k):
    """(40, 100): the element-wise X path (k % 8 != 0) with a ragged last tile row; (200, 104): a second workgroup of units, the 16-byte
    X path on the contiguous x."""
    for out_dtype in DTYPES:
        _contract_holds(COUNT, n, k, ROUTINGS["mixed"], 600 + n, out_dtype, (0, 2))


def test_a_long_run_bit_for_bit():
    assert -(-2100 // 32) == 66                                      # a second 64-tile strided hand-out at split 1
    _contract_holds(2, 72, 2100, (0, 2, 35), 700, "float32", (1, 0), views=False)


def test_the_bytes_of_padding_k_rows_mean_nothing():
    """k = 100: k-rows 100..127 of every expert's last tile row are padding.  Their code and exponent bytes are overwritten with 0xFF in
    a copy of the arena: Y keeps every bit."""
    n, k, rows = 40, 100, ROUTINGS["mixed"]
    pts, _ref, x, _view, bias = _case(COUNT, n, k, rows[-1], 640)
    batch = packed.batch_of(pts)
    dirty = batch.arena.clone()
    for e, pt in enumerate(pts):
        tiles_h, tiles_w = pt.map.shape
        for tc in range(tiles_w):
            t = (tiles_h - 1) * tiles_w + tc
            f, base = int(pt.map[tiles_h - 1, tc]), (int(batch.bases[e]) + int(pt.offsets[t])) * 64
            g0 = 2 * (k - 32 * (tiles_h - 1))                        # the first padding group: k-row 4 of the tile
            if f == 0:
                dirty[base + 32 * g0: base + 2048] = 0xFF
            else:
                per = {1: 16, 2: 8, 3: 4}[f]
                dirty[base + g0: base + 64] = 0xFF
                dirty[base + 64 + per * g0: base + TILE_BYTES[f]] = 0xFF
    assert int((dirty != batch.arena).sum()) > COUNT * 2 * 28 * 4
    for kernel, (fn, _size) in ENTRIES.items():
        for split in (0, 1, 2):
            for dtype in DTYPES.values():
                clean = _call(kernel, pts, x, rows, bias, dtype, split)
                got = fn(x, _rows_dev(rows), dirty, batch.maps_dev, batch.offsets_dev, batch.bases_dev, COUNT, n, bias=bias, out_dtype=dtype, split=split)
                _same(got, clean, False, (kernel, split, dtype))


# ----------------------------------------------------------------------------- exact arithmetic, independent of every other kernel

@functools.lru_cache(maxsize=None)
def _grid_experts(count=COUNT, n=N, k=K, T=200, seed=4242):
    """(experts, P̂ float64 (count, k, n) from the oracle, bias float32 (count, n), x float32 (T, k)) on the integer grid; preconditions
    asserted on the CPU - made once, never written."""
    rng = np.random.default_rng(seed)
    w = (rng.integers(-255, 256, size=(count, n, k)) * GRID).astype(np.float32)
    b = (rng.integers(-255, 256, size=(count, n)) * GRID).astype(np.float32)
    x = rng.integers(-4, 5, size=(T, k)).astype(np.float32)
    maps = np.stack([random_map((k, n), seed + 40 + i) for i in range(count)])
    phat = np.stack([_phat(w[i], maps[i]) for i in range(count)])
    for i in range(count):
        _grid_preconditions(x, phat[i].T, b[i].astype(np.float64))
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")
    for a in (phat, b, x):
        a.setflags(write=False)
    return pts, phat, b, x


def _product(phat, b, x, ranges, T, fill=0.0):
    """float64: x[r0:r1] @ phat[e] + b[e] over `ranges` [(e, r0, r1)], `fill` elsewhere; exact in float32."""
    want = np.full((T, phat.shape[2]), fill, dtype=np.float64)
    for e, r0, r1 in ranges:
        want[r0:r1] = x[r0:r1].astype(np.float64) @ phat[e] + (0.0 if b is None else b[e].astype(np.float64)[None, :])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return want


def _ranges(rows):
    return [(e, rows[e], rows[e + 1]) for e in range(len(rows) - 1)]


def test_the_integer_grid_equals_the_float64_product_at_every_split():
    rows = ROUTINGS["hot"]
    pts, phat, b, x = _grid_experts()
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for bias_h, bias_d in ((None, None), (b, bd)):
        want = _product(phat, bias_h, x, _ranges(rows), rows[-1])
        emu = packed.matmul_grouped(x, list(rows), pts, bias=bias_h, backend="emulation")
        assert np.array_equal(emu.astype(np.float64), want)
        for kernel in ENTRIES:
            for split in (0, 1, 2, 13):
                got = packed.matmul_grouped(xd, list(rows), pts, bias=bias_d, split=split, kernel=kernel).cpu().numpy()
                assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (kernel, split, np.argwhere(got != want)[:4])
            half = packed.matmul_grouped(xd, _rows_dev(rows), pts, bias=bias_d, out_dtype="bfloat16", kernel=kernel)
            assert torch.equal(half.cpu(), torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)), kernel


def test_one_hot_rows_return_the_last_expert_and_a_flipped_byte_shows_at_its_position():
    s, last = 3, COUNT - 1
    w = np.stack([gen("normal_f32", 820 + i, (N, K)) for i in range(COUNT)])
    maps = np.stack([random_map((K, N), 830 + i) for i in range(COUNT)])
    maps[last, -1, -1] = 1                                   # bfp8 in the last tile, ragged in both directions
    pts = packed.pack_batch_transposed(torch.from_numpy(w).cuda(), maps, backend="hip")          # this test's own arena: a byte of it is flipped
    rows = [0, 0, 0, 0, 0, K]                                # the last expert sees 2ˢ·I_k: ten chunks
    xd = _x_dev(np.eye(K, dtype=np.float32) * np.float32(2.0 ** s))
    want = (2.0 ** s) * _phat(w[last], maps[last])
    assert np.all(np.isfinite(want)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    tr, tc, r, c = maps.shape[1] - 1, maps.shape[2] - 1, 4, 5
    assert 32 * tr + r < K and 32 * tc + c < N
    at, mask = _code_byte(pts[last], tr, tc, r, c)
    for flipped in (False, True):
        if flipped:
            pts[last].data[at] ^= mask                       # a slice of the arena
        for kernel in ENTRIES:
            for split in (1, 0):
                y = packed.matmul_grouped(xd, rows, pts, split=split, kernel=kernel).cpu().numpy().astype(np.float64)
                bad = np.argwhere(y != want)
                assert [tuple(v) for v in bad] == ([(32 * tr + r, 32 * tc + c)] if flipped else []), (flipped, kernel, split, bad[:6])


def test_three_hundred_groups_take_the_plan_and_the_search_past_one_window():
    """count = 300 > 256 threads of the plan kernel and > 64 entries of the search's last window; groups of 0, 1 and 40 rows in turn."""
    count, n, k = 300, 40, 64
    sizes = [(0, 1, 40)[e % 3] for e in range(count)]
    rows = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    T = rows[-1]
    pts, phat, b, x = _grid_experts(count, n, k, T, 77)
    want = _product(phat, b, x, _ranges(rows), T)
    xd, bd = _x_dev(x.copy()), torch.from_numpy(b.copy()).cuda()
    for kernel in ENTRIES:
        for split in (0, 2):
            got = packed.matmul_grouped(xd, _rows_dev(rows), pts, bias=bd, split=split, kernel=kernel).cpu().numpy().astype(np.float64)
            assert np.array_equal(got, want), (kernel, split, np.argwhere(got != want)[:4])


# ----------------------------------------------------------------------------- guards over buffers that stay whole

def _zeroed(phat, e, tiles_w, tiles):
    out = phat.copy()
    for t in tiles:
        tr, tc = divmod(int(t), tiles_w)
        out[e, 32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = 0.0
    return out


def _guarded(kernel, pts, x, b, rows, split, arena=None, maps_dev=None, bases_dev=None):
    """The entry with sentinel rows behind X and Y and sentinel bytes behind the workspace → Y's T rows as float64; the sentinels hold."""
    batch = packed.batch_of(pts)
    T, k, n, pad = x.shape[0], batch.rows, batch.cols, 16
    fn, size = ENTRIES[kernel]
    xbuf = torch.full((T + pad, k), 3.0, dtype=torch.bfloat16, device="cuda")
    xbuf[:T] = _x_dev(x.copy())
    ybuf = torch.full((T + pad, n), -7.0, dtype=torch.float32, device="cuda")
    need = size(T, batch.count, n, k, split)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    fn(xbuf[:T], _rows_dev(rows), batch.arena if arena is None else arena, batch.maps_dev if maps_dev is None else maps_dev, batch.offsets_dev,
       batch.bases_dev if bases_dev is None else bases_dev, batch.count, n, bias=None if b is None else torch.from_numpy(b.copy()).cuda(),
       split=split, out=ybuf[:T], workspace=ws[:need] if need else None)
    assert bool((ybuf[T:] == -7.0).all()) and bool((ws[need:] == 0xFF).all()) and bool((xbuf[T:] == 3.0).all()), (kernel, split)
    return ybuf[:T].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("kernel", list(ENTRIES))
def test_blobs_outside_their_stream_and_codes_that_are_no_format_multiply_as_zeros(kernel):
    rows = ROUTINGS["hot"]
    pts, phat, b, x = _grid_experts()
    batch = packed.batch_of(pts)
    tiles_h, tiles_w = pts[0].map.shape
    tiles = tiles_h * tiles_w
    last = COUNT - 2                                         # the last group WITH rows on this routing
    # packed_bytes cut short of that expert's last tile (and of everything behind it, which has no rows)
    cut = (int(batch.bases[last]) + int(pts[last].offsets[tiles - 1])) * 64 + 64
    assert COUNT * tiles * TILE_BYTES[3] <= cut < batch.arena.numel()
    short = batch.arena[:cut]                                # the buffer stays whole: a kernel without the guard reads real bytes
    assert short.data_ptr() == batch.arena.data_ptr()
    left = _zeroed(phat, last, tiles_w, [tiles - 1])
    assert np.count_nonzero(left != phat) > 0
    for split in (1, 2, 0):
        for bias in (None, b):
            got = _guarded(kernel, pts, x, bias, rows, split, arena=short)
            want = _product(left, bias, x, _ranges(rows), rows[-1], fill=-7.0)
            assert np.array_equal(got, want), ("packed_bytes", split, bias is not None, np.argwhere(got != want)[:4])
    # one group's stream cut short by its own bases: the group behind it now starts a unit early and reads bytes that mean nothing
    e = 1
    bases = batch.bases_dev.clone()
    bases[e + 1] -= 1
    left = _zeroed(phat, e, tiles_w, [tiles - 1])
    for split in (1, 2):
        got = _guarded(kernel, pts, x, b, rows, split, bases_dev=bases)
        want = _product(left, b, x, _ranges(rows), rows[-1], fill=-7.0)
        for g in (0, 1, 3, 4):
            assert np.array_equal(got[rows[g]:rows[g + 1]], want[rows[g]:rows[g + 1]]), ("bases", split, g)
    assert np.array_equal(batch.bases_dev.cpu().numpy().view(np.uint64), batch.bases)            # the shared tables were not touched
    # map codes 4 and -1, in ring rounds 1 and 2 of their runs at split 1
    t_first, t_second = 3 * tiles_w + 0, 9 * tiles_w + 2
    maps = batch.maps_dev.clone()
    maps[e, t_first] = 4
    maps[e, t_second] = -1
    left = _zeroed(phat, e, tiles_w, (t_first, t_second))
    for split in (1, 2, 0):
        got = _guarded(kernel, pts, x, b, rows, split, maps_dev=maps)
        want = _product(left, b, x, _ranges(rows), rows[-1], fill=-7.0)
        assert np.array_equal(got, want), ("codes", split, np.argwhere(got != want)[:4])


T0 = ROUTINGS["mixed"][-1]
# (what group_rows holds, the groups whose clamped range overlaps no other and is computed in full)
BAD_ROWS = {
    "decreasing": ([0, 3, 3, 35, 20, 20], (0, 2)),
    "overlapping": ([0, 40, 20, 50, 60, 70], (3, 4)),        # groups 0 (0..40) and 2 (20..50) overlap: their rows are unspecified
    "past-T": ([0, 3, 3, 35, 36, T0 + 9], (0, 2, 3, 4)),
    "negative": ([-5, 3, 3, 35, 36, T0], (0, 2, 3, 4)),
    "no-group": ([0, 3, 3, 10, 40, 41], (0, 2, 3, 4)),       # rows 41.. belong to no group
}


@pytest.mark.parametrize("kernel", list(ENTRIES))
@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_group_rows_are_clamped_before_any_use(name, kernel):
    rows, right = BAD_ROWS[name]
    pts, phat, b, x = _grid_experts()
    x = x[:T0]
    r0, r1 = packed.clamp_group_rows(rows, T0)
    written = np.zeros(T0, dtype=bool)
    for e in range(COUNT):
        written[r0[e]:r1[e]] = True
    for split in (1, 2):
        got = _guarded(kernel, pts, x, b, rows, split)
        for e in right:
            want = x[r0[e]:r1[e]].astype(np.float64) @ phat[e] + b[e].astype(np.float64)[None, :]
            assert np.array_equal(got[r0[e]:r1[e]], want), (name, split, e)
        assert np.all(got[~written] == -7.0), (name, split, "a row of no clamped group was written")
    if name in ("decreasing", "overlapping"):
        return
    rows_dev = _rows_dev(rows)                               # the emulation given the device array applies the same rule: rows of no group are zeros
    emu = packed.matmul_grouped(x, rows_dev, pts, bias=b, backend="emulation")
    dev = packed.matmul_grouped(_x_dev(x.copy()), rows_dev, pts, bias=torch.from_numpy(b.copy()).cuda(), kernel=kernel).cpu().numpy()
    assert np.array_equal(emu, dev) and (name != "no-group" or not emu[41:].any()), name


# ----------------------------------------------------------------------------- the module and the batch forms

def test_the_module_keeps_one_workspace_and_the_batch_forms_agree():
    rows = ROUTINGS["mixed"]
    pts, _ref, x, _view, bias = _case(COUNT, N, K, rows[-1], 500)
    small = [0, 1, 1, 3, 4, 5]
    for kernel, (_fn, size) in ENTRIES.items():
        for out_dtype in DTYPES:
            mod = packed.PackedExpertsMatmul(pts, bias=bias, out_dtype=out_dtype, kernel=kernel)
            assert mod.backend == "hip" and mod.batch is packed.batch_of(pts) and (mod.in_features, mod.out_features) == (K, N)
            for r, xs in ((list(rows), x), (small, x[:5]), (list(rows), x)):
                want = packed.matmul_grouped(xs, r, pts, bias=bias, out_dtype=out_dtype, kernel=kernel)
                assert np.array_equal(_bits(mod(xs, r)).cpu().numpy(), _bits(want).cpu().numpy()), (kernel, out_dtype, len(xs))
            assert mod._workspace is not None and mod._workspace.numel() == size(rows[-1], COUNT, N, K, 0)
            none = mod(x, torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))                  # every group empty: zeros
            assert tuple(none.shape) == (rows[-1], N) and not bool(none.any())
    assert _eff(rows[-1], COUNT, N, K, 0) > 1
    # matmul_batch is the grouped call
    m = 4
    x3 = x[:COUNT * m].reshape(COUNT, m, K)
    y3 = packed.matmul_batch(x3, pts, bias=bias, split=2, kernel="chunks")
    want = packed.matmul_grouped(x[:COUNT * m], [m * e for e in range(COUNT + 1)], pts, bias=bias, split=2)
    assert tuple(y3.shape) == (COUNT, m, N) and torch.equal(_bits(y3.reshape(COUNT * m, N)), _bits(want))
    # a batch rebuilt by as_batch from the same tensors gives the same bits
    loaded = [packed.PackedTensor(pt.shape, pt.shape_info, pt.rows, pt.cols, pt.map, pt.offsets, pt.data.clone()) for pt in pts]
    assert packed.batch_of(loaded) is None
    again = packed.as_batch(loaded)
    assert again is not packed.batch_of(pts) and torch.equal(again.arena, packed.batch_of(pts).arena)
    for kernel in ENTRIES:
        assert torch.equal(_bits(packed.matmul_grouped(x, list(rows), again, bias=bias, kernel=kernel)),
                           _bits(packed.matmul_grouped(x, list(rows), pts, bias=bias, kernel=kernel))), kernel
    for out_dtype, dtype in DTYPES.items():
        empty = packed.matmul_grouped(x[:0], [0] * (COUNT + 1), pts, out_dtype=out_dtype)
        assert tuple(empty.shape) == (0, N) and empty.dtype == dtype and empty.is_cuda
