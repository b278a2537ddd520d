"""GPU: the packed kernels of csrc/mtq_packed.hip where an address passes 32 bits.  The kernels form byte offsets in uint64_t and element
indices in int64_t; nothing but reading said so.  Nothing here computes anything large: the tensors stay at (n, k) = (70, 100) with
m = 33 and (200, 300) with m = 300 on the integer grid of tests/packed_cases.py (Y EQUALS the float64 product, Ŵ is the oracle's), and
only their PLACES are far: one buffer from torch.empty, never filled whole, holds whatever a test puts past byte 2³² of it.

FAR = 2²⁶ + 1027 units of 64 bytes is byte 4 GiB + 65 728: 64-byte aligned, no power of two, and (64·FAR) mod 2³² = 65 728, so an offset
cut to 32 bits lands inside the same buffer, where a decoy waits: the stream of −W under the same map (a wrap gives −Y, not a fault).

  * single-tensor tables whose every offset is FAR units on (PackedTables built by hand from a real pack's map, nbytes set as the guard
    tests set it): unpack, block, wide and skinny (splits 1 and 2) give what the unshifted tables give, the oracle's bits and the
    float64 product; pack writes the encoder's bytes at byte 64·FAR and leaves a sentinel window around the wrapped place alone;
  * an arena with hand-made bases [1027, FAR, FAR + len₁ + 5, end] (gaps are legal): pack_tiles_batched writes expert 0 low, where
    expert 1 would wrap to (expert 0 is −W₁ under expert 1's map: the decoy), and experts 1 and 2 past 4 GiB with the gap between them
    untouched; unpack_tiles_batched and the grouped linear (groups of 3, 35 and 32 rows, splits 1 and 2) equal the oracle per expert;
  * the guard in 64 bits: packed_bytes / the arena's length 64 bytes short of the end of the last far blob: that tile alone reads as
    zeros (linear) or is not stored (unpack), through unpack, block, wide, skinny and grouped, over buffers that stay whole;
  * packed_offsets_device over 131 080 maps of 1024 bf16 tiles: bases pass 2³² units and equal NumPy's uint64 cumulative sum;
  * matrix indices: X (300 × 300 bf16) and Y (bf16) as views with a row pitch of 2²³ + 8 elements, so rows from 256 on start past element
    2³¹ and byte 2³²; Y float32 at pitch 2²² + 8 (rows from 256 on past byte 2³²) and, 257 rows, at pitch 2²³ + 8 (row 256 past element
    2³¹: 8.0 GiB); block and wide with each as input or output, grouped over T = 300 rows of such an X in groups of 100, 0 and 200;
    pack_tiles_batched reads, and unpack_tiles_batched writes, five 70 × 100 bf16 matrices at a matrix stride of 2²⁹ + 64 elements.

At most one big buffer is alive at a time (5.4 GB for all but the last test, 8.6 GB there: under 9 GiB of device memory at any moment);
torch.cuda.OutOfMemoryError from that allocation is the module's only skip.
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
from tests.packed_cases import TILE_BYTES, _grid_case, _grid_preconditions, expected_bits, random_map

pytestmark = pytest.mark.gpu

FAR = 2 ** 26 + 1027                                 # units of 64 bytes
WRAP = (64 * FAR) % 2 ** 32                          # where byte 64·FAR lands when cut to 32 bits
PITCH_16 = 2 ** 23 + 8                               # row pitch in elements: row 256 starts past element 2³¹
PITCH_32 = 2 ** 22 + 8                               # float32: row 256 starts past byte 2³²
MATRIX_STRIDE = 2 ** 29 + 64                         # matrix 4 starts past element 2³¹
USUAL = 2 * (4 * MATRIX_STRIDE + 70 * 100) + 4096    # bytes: the largest need of every test but the last
SHAPES = [(33, 70, 100), (300, 200, 300)]
LOW, HIGH = 0xA5, 0x5A                               # sentinel bytes around the wrapped and the far places
assert WRAP == 65728 and 64 * FAR == 2 ** 32 + WRAP and FAR % 2 == 1


class _Big:
    """The one big device buffer: grown by dropping the old one first, so two are never alive together."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes: int):
        nbytes = max(int(nbytes), USUAL)
        if self.buf is None or self.buf.numel() < nbytes:
            self.release()
            try:
                self.buf = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            except torch.cuda.OutOfMemoryError:
                pytest.skip(f"out of device memory for the {nbytes}-byte buffer of the far-address tests (the only permitted skip)")
        assert self.buf.data_ptr() % 256 == 0
        return self.buf

    def release(self):
        self.buf = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    holder = _Big()
    yield holder
    holder.release()


def _what(w, amap):
    return expected_bits(w, amap).view(np.float32).astype(np.float64)


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _x_dev(x):
    assert np.array_equal(to_bf16_valued(x), x)
    return torch.from_numpy(np.array(x)).to(torch.bfloat16).cuda()                # a copy: x may be read-only


def _zeroed(what, tiles_w, tiles):
    out = what.copy()
    for t in tiles:
        tr, tc = divmod(int(t), tiles_w)
        out[32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """(x, w, b, map, Ŵ float64, the packed W, the packed −W under the same map) — made once, never written to."""
    x, w, b = _grid_case(m, n, k, 9000 + n + k)
    amap = random_map((n, k), 9100 + n)
    what = _what(w, amap)
    _grid_preconditions(x, what, b.astype(np.float64))
    pt, decoy = packed.pack(w, amap, backend="hip"), packed.pack(-w, amap, backend="hip")
    assert pt.nbytes == decoy.nbytes and not torch.equal(pt.data, decoy.data)
    for a in (x, w, b, what):
        a.setflags(write=False)
    return x, w, b, amap, what, pt, decoy


def _far_tables(pt, nbytes):
    """pt's tables with every offset FAR units on and packed_bytes = nbytes."""
    off = pt.offsets.astype(np.uint64) + np.uint64(FAR)
    assert int(off.max()) < 2 ** 32 and int(off.min()) * 64 >= 2 ** 32
    tables = hb.PackedTables(pt.map, pt.tables().map_dev, torch.from_numpy(off.astype(np.uint32).view(np.int32)).cuda())
    assert tables.nbytes == pt.nbytes
    tables.nbytes = int(nbytes)
    return tables


def _placed(big, pt, decoy):
    """The big buffer's first 64·FAR + len bytes with the real stream at byte 64·FAR and the decoy at the wrapped place."""
    data = big.get(64 * FAR + pt.nbytes)[:64 * FAR + pt.nbytes]
    data[64 * FAR:] = pt.data
    data[WRAP:WRAP + decoy.nbytes] = decoy.data
    return data


def _want_y(x, what, b, with_bias):
    want = x.astype(np.float64) @ what.T + (b.astype(np.float64)[None, :] if with_bias else 0.0)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return want


def _linears(xd, data, tables, n, bias, dtype):
    """{name: Y} of every single-tensor linear through `tables`: block and wide on all rows, skinny (splits 1 and 2) on the first 32."""
    out = {"block": hb.packed_linear(xd, data, tables, n, bias=bias, out_dtype=dtype),
           "wide": hb.packed_linear_wide(xd, data, tables, n, bias=bias, out_dtype=dtype)}
    for split in (1, 2):
        out[f"skinny, split {split}"] = hb.packed_linear_skinny(xd[:32], data, tables, n, bias=bias, out_dtype=dtype, split=split)
    return out


def _check_linears(x, what, b, data, tables, n, near=None):
    """Every linear through (data, tables) EQUALS the float64 product with `what`; `near`: (data, tables) that must give the same bits."""
    xd, bd = _x_dev(x), torch.from_numpy(b.copy()).cuda()
    for with_bias in (False, True):
        want = _want_y(x, what, b, with_bias)
        want_bf16 = torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)
        for dtype in (torch.float32, torch.bfloat16):
            got = _linears(xd, data, tables, n, bd if with_bias else None, dtype)
            ref = _linears(xd, near[0], near[1], n, bd if with_bias else None, dtype) if near else {}
            for name, y in got.items():
                rows = y.shape[0]
                if dtype == torch.float32:
                    g = y.cpu().numpy().astype(np.float64)
                    assert np.array_equal(g, want[:rows]), (name, with_bias, np.argwhere(g != want[:rows])[:4])
                else:
                    assert np.array_equal(_ints(y).cpu().numpy(), _ints(want_bf16[:rows]).numpy()), (name, with_bias)
                if near:
                    assert torch.equal(_ints(y), _ints(ref[name])), (name, with_bias, dtype, "differs from the unshifted tables' bits")


# ----------------------------------------------------------------------------- single-tensor tables at a far offset

@pytest.mark.parametrize("m,n,k", SHAPES)
def test_tables_at_a_far_offset_read_the_far_stream(big, m, n, k):
    x, w, b, amap, what, pt, decoy = _case(m, n, k)
    data = _placed(big, pt, decoy)
    far = _far_tables(pt, data.numel())
    want = expected_bits(w, amap)
    for dtype in (torch.float32, torch.bfloat16):
        y = hb.unpack_tiles(data, far, n, k, dtype=dtype)
        assert torch.equal(_ints(y), _ints(hb.unpack_tiles(pt.data, pt.tables(), n, k, dtype=dtype))), dtype
        bits = y.view(torch.int32).cpu().numpy().view(np.uint32) if dtype == torch.float32 else _ints(y).cpu().numpy().view(np.uint16).astype(np.uint32) << np.uint32(16)
        assert np.array_equal(bits, want), (dtype, np.argwhere(bits != want)[:4])
    _check_linears(x, what, b, data, far, n, near=(pt.data, pt.tables()))
    # the decoy is one: through unshifted tables the bytes at the wrapped place multiply to the product with the oracle's Ŵ of −W
    low = hb.packed_linear(_x_dev(x), data[WRAP:WRAP + decoy.nbytes], pt.tables(), n).cpu().numpy().astype(np.float64)
    assert np.array_equal(low, x.astype(np.float64) @ _what(-w, amap).T) and np.any(low != _want_y(x, what, b, False))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_pack_through_far_tables_writes_at_the_far_place_only(big, m, n, k):
    _x, w, _b, amap, _what64, pt, _decoy = _case(m, n, k)
    data = big.get(64 * FAR + pt.nbytes)[:64 * FAR + pt.nbytes]
    far = _far_tables(pt, data.numel())
    pad = 4096
    data[WRAP - pad:WRAP + pt.nbytes + pad] = LOW
    data[64 * FAR - pad:] = HIGH
    got = hb.pack_tiles(torch.from_numpy(np.array(w)).cuda(), far, out=data)
    assert got.data_ptr() == data.data_ptr()
    enc = packed.pack(w, amap, backend="emulation")
    assert np.array_equal(data[64 * FAR:].cpu().numpy(), enc.data) and torch.equal(data[64 * FAR:], pt.data)
    assert bool((data[WRAP - pad:WRAP + pt.nbytes + pad] == LOW).all()), "bytes around the wrapped place were written"
    assert bool((data[64 * FAR - pad:64 * FAR] == HIGH).all())


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_the_guard_holds_in_64_bits(big, m, n, k):
    x, w, b, amap, what, pt, decoy = _case(m, n, k)
    data = _placed(big, pt, decoy)
    tiles_h, tiles_w = amap.shape
    last = tiles_h * tiles_w - 1
    assert int(pt.offsets[last]) * 64 + TILE_BYTES[int(amap.reshape(-1)[last])] == pt.nbytes
    short = _far_tables(pt, data.numel() - 64)         # 64 bytes short of the end of the last tile; the buffer stays whole
    assert short.nbytes >= (last + 1) * TILE_BYTES[3]
    near = copy.copy(pt.tables())
    near.nbytes = pt.nbytes - 64
    _check_linears(x, _zeroed(what, tiles_w, (last,)), b, data, short, n, near=(pt.data, near))
    want = expected_bits(w, amap)
    y = torch.full((n, k), -7.0, dtype=torch.float32, device="cuda")
    hb.unpack_tiles(data, short, n, k, out=y)
    yb = y.cpu().numpy()
    in_last = np.zeros((n, k), dtype=bool)
    in_last[32 * (tiles_h - 1):, 32 * (tiles_w - 1):] = True
    assert np.array_equal(yb.view(np.uint32)[~in_last], want[~in_last]) and np.all(yb[in_last] == -7.0)
    assert pt.tables().nbytes == pt.nbytes             # the shared tables were not touched


# ----------------------------------------------------------------------------- arena bases at a far offset

@functools.lru_cache(maxsize=None)
def _arena_case():
    """Three experts of (70, 100): expert 0 is −W₁ under expert 1's map (it lies where expert 1 would wrap to)."""
    n, k = 70, 100
    x, w1, b1 = _grid_case(70, n, k, 9500)
    _x2, w2, b2 = _grid_case(1, n, k, 9501)
    m1, m2 = random_map((n, k), 9502), random_map((n, k), 9503)
    w, maps, b = np.stack([-w1, w1, w2]), np.stack([m1, m1, m2]), np.stack([b2, b1, b2])
    what = np.stack([_what(w[e], maps[e]) for e in range(3)])
    for e in range(3):
        _grid_preconditions(x, what[e], b[e].astype(np.float64))
    enc = [packed.pack(w[e], maps[e], backend="emulation").data for e in range(3)]
    for a in (x, w, b, what):
        a.setflags(write=False)
    return n, k, x, w, b, maps, what, enc


def _arena(big):
    """The packed arena on hand-made far bases → (arena, maps_dev, offsets_dev, bases_dev, bases, lens), checked byte for byte."""
    n, k, _x, w, _b, maps, _what64, enc = _arena_case()
    tiles = maps[0].size
    maps_dev = torch.from_numpy(maps.reshape(3, tiles)).cuda()
    offsets_dev, _own, bad = hb.packed_offsets_device(maps_dev, 3, tiles)
    assert not bad.cpu().numpy().any()
    lens = [e.size // 64 for e in enc]
    assert offsets_dev[:, -1].cpu().tolist() == lens and lens[0] == lens[1]
    bases = [1027, FAR, FAR + lens[1] + 5, FAR + lens[1] + 5 + lens[2]]
    assert 64 * bases[0] == WRAP                      # expert 0 lies exactly where expert 1's base wraps to
    bases_dev = torch.tensor(bases, dtype=torch.int64, device="cuda")
    arena = big.get(64 * bases[3])[:64 * bases[3]]
    low_end = 64 * (bases[0] + lens[0] + 5 + lens[2] + 64)
    pad = 4096
    arena[:low_end] = LOW
    arena[64 * FAR - pad:] = HIGH
    hb.pack_tiles_batched(torch.from_numpy(np.array(w)).cuda(), maps_dev, offsets_dev, bases_dev, arena)
    for e in range(3):
        got = arena[64 * bases[e]:64 * (bases[e] + lens[e])].cpu().numpy()
        assert np.array_equal(got, enc[e]), (e, np.flatnonzero(got != enc[e])[:8])
    assert bool((arena[:WRAP] == LOW).all()) and bool((arena[WRAP + enc[0].size:low_end] == LOW).all()), "bytes at a wrapped place were written"
    assert bool((arena[64 * FAR - pad:64 * FAR] == HIGH).all()) and bool((arena[64 * (bases[1] + lens[1]):64 * bases[2]] == HIGH).all())
    # the decoy of expert 2 where its base wraps to: −W₂ under its map
    wrap2 = (64 * bases[2]) % 2 ** 32
    assert wrap2 == 64 * (1027 + lens[1] + 5) and wrap2 + enc[2].size <= low_end
    arena[wrap2:wrap2 + enc[2].size] = torch.from_numpy(packed.pack(-w[2], maps[2], backend="emulation").data).cuda()
    return arena, maps_dev, offsets_dev, bases_dev, bases, lens


GROUP_ROWS = (0, 3, 38, 70)                          # groups of 3, 35 and 32 rows


def _check_arena_reads(arena, maps_dev, offsets_dev, bases_dev, what, gone=None):
    """unpack_tiles_batched and the grouped linear over `arena` against the oracle per expert; gone = (expert, tile): not there."""
    n, k, x, w, b, maps, _what64, _enc = _arena_case()
    tiles_w = maps[0].shape[1]
    for dtype in (torch.float32, torch.bfloat16):
        y = torch.full((3, n, k), -7.0, dtype=dtype, device="cuda")
        hb.unpack_tiles_batched(arena, maps_dev, offsets_dev, bases_dev, 3, n, k, dtype, out=y)
        for e in range(3):
            want = expected_bits(w[e], maps[e])
            bits = y[e].view(torch.int32).cpu().numpy().view(np.uint32) if dtype == torch.float32 else _ints(y[e]).cpu().numpy().view(np.uint16).astype(np.uint32) << np.uint32(16)
            inside = np.ones((n, k), dtype=bool)
            if gone is not None and gone[0] == e:
                tr, tc = divmod(gone[1], tiles_w)
                inside[32 * tr:32 * tr + 32, 32 * tc:32 * tc + 32] = False
                assert np.all(y[e].float().cpu().numpy()[~inside] == -7.0), (e, dtype, "a tile that is not there was stored")
            assert np.array_equal(bits[inside], want[inside]), (e, dtype, np.argwhere((bits != want) & inside)[:4])
    xd, bd = _x_dev(x), torch.from_numpy(np.array(b)).cuda()
    rows_dev = torch.tensor(GROUP_ROWS, dtype=torch.int32, device="cuda")
    for with_bias in (False, True):
        want = np.zeros((70, n))
        for e in range(3):
            r0, r1 = GROUP_ROWS[e], GROUP_ROWS[e + 1]
            want[r0:r1] = _want_y(x[r0:r1], what[e], b[e], with_bias)
        want_bf16 = torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16)
        for split in (1, 2):
            for dtype in (torch.float32, torch.bfloat16):
                y = hb.packed_linear_skinny_grouped(xd, rows_dev, arena, maps_dev, offsets_dev, bases_dev, 3, n, bias=bd if with_bias else None,
                                                    out_dtype=dtype, split=split)
                if dtype == torch.float32:
                    g = y.cpu().numpy().astype(np.float64)
                    assert np.array_equal(g, want), (with_bias, split, np.argwhere(g != want)[:4])
                else:
                    assert np.array_equal(_ints(y).cpu().numpy(), _ints(want_bf16).numpy()), (with_bias, split)


def test_arena_bases_at_a_far_offset(big):
    arena, maps_dev, offsets_dev, bases_dev, bases, _lens = _arena(big)
    assert arena.numel() == 64 * bases[3] > 2 ** 32
    _check_arena_reads(arena, maps_dev, offsets_dev, bases_dev, _arena_case()[6])


def test_the_arenas_guard_holds_in_64_bits(big):
    arena, maps_dev, offsets_dev, bases_dev, bases, _lens = _arena(big)
    maps, what = _arena_case()[5], _arena_case()[6]
    last = maps[2].size - 1
    short = arena[:arena.numel() - 64]                 # the buffer stays whole: a kernel without the guard reads real bytes
    assert short.data_ptr() == arena.data_ptr() and short.numel() >= 3 * maps[0].size * TILE_BYTES[3]
    left = what.copy()
    left[2] = _zeroed(what[2], maps[2].shape[1], (last,))
    assert np.count_nonzero(left != what) > 0
    _check_arena_reads(short, maps_dev, offsets_dev, bases_dev, left, gone=(2, last))


# ----------------------------------------------------------------------------- bases past 2³² units

def test_device_bases_pass_32_bits_of_units():
    count, tiles = 131080, 1024
    maps_dev = torch.zeros((count, tiles), dtype=torch.int8, device="cuda")             # all bf16: 32 units a tile, 32 768 a map
    offsets, bases, bad = hb.packed_offsets_device(maps_dev, count, tiles)
    want = np.cumsum(np.concatenate([[0], np.full(count, tiles * TILE_BYTES[0] // 64)]).astype(np.uint64))
    assert want.dtype == np.uint64 and int(want[-1]) == count * 32768 > 2 ** 32
    got = bases.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:4]
    row = torch.from_numpy(hb.packed_offsets(np.zeros(tiles, dtype=np.int8)).view(np.int32)).cuda()
    assert tuple(offsets.shape) == (count, tiles + 1) and bool((offsets == row[None, :]).all())
    assert not bool(bad.any())


# ----------------------------------------------------------------------------- matrix indices past 2³¹ elements

def _rows_view(big, dtype, rows, cols, pitch):
    """A (rows, cols) view of the big buffer with a row pitch of `pitch` elements."""
    esz = 2 if dtype == torch.bfloat16 else 4
    buf = big.get(((rows - 1) * pitch + cols) * esz + 64)
    view = torch.as_strided(buf.view(dtype), (rows, cols), (pitch, 1))
    assert view.data_ptr() == buf.data_ptr() and view[256:].data_ptr() - buf.data_ptr() >= 2 ** 32
    return view


def _same_rows(got, want, what):
    """got, want: host arrays (m, n); the message names rows 255 and 256, the two sides of element 2³¹ / byte 2³²."""
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, f"row 255 {'differs' if 255 in bad else 'is right'}, row 256 {'differs' if 256 in bad else 'is right'}", bad[:8])


@pytest.mark.parametrize("entry", ["block", "wide"])
def test_x_rows_past_element_2_31(big, entry):
    m, n, k = 300, 200, 300
    x, _w, b, _amap, what, pt, _decoy = _case(m, n, k)
    xv = _rows_view(big, torch.bfloat16, m, k, PITCH_16)
    assert 256 * PITCH_16 > 2 ** 31
    xv.copy_(_x_dev(x))
    fn = hb.packed_linear if entry == "block" else hb.packed_linear_wide
    y = fn(xv, pt.data, pt.tables(), n, bias=torch.from_numpy(b.copy()).cuda()).cpu().numpy().astype(np.float64)
    _same_rows(y, _want_y(x, what, b, True), (entry, "X at a far pitch"))


@pytest.mark.parametrize("entry", ["block", "wide"])
@pytest.mark.parametrize("dtype,pitch,m", [(torch.bfloat16, PITCH_16, 300), (torch.float32, PITCH_32, 300)], ids=["bf16", "float32"])
def test_y_rows_past_byte_2_32(big, entry, dtype, pitch, m):
    _y_at_a_far_pitch(big, entry, dtype, pitch, m)


def _y_at_a_far_pitch(big, entry, dtype, pitch, m):
    n, k = 200, 300
    x, _w, b, _amap, what, pt, _decoy = _case(300, n, k)
    yv = _rows_view(big, dtype, m, n, pitch)
    yv.fill_(-7.0)
    fn = hb.packed_linear if entry == "block" else hb.packed_linear_wide
    got = fn(_x_dev(x[:m]), pt.data, pt.tables(), n, bias=torch.from_numpy(b.copy()).cuda(), out_dtype=dtype, out=yv)
    assert got.data_ptr() == yv.data_ptr()
    want = torch.from_numpy(_want_y(x[:m], what, b, True).astype(np.float32)).to(dtype)
    _same_rows(_ints(yv.contiguous()).cpu().numpy(), _ints(want).numpy(), (entry, dtype, pitch, "Y at a far pitch"))


def test_grouped_x_rows_past_element_2_31(big):
    n, k, T = 200, 300, 300
    x, w0, b0, amap0, what0, _pt, _decoy = _case(T, n, k)
    ws, bs, maps = [np.array(w0)], [np.array(b0)], [amap0]
    for e in (1, 2):
        _x0, w, b = _grid_case(1, n, k, 9600 + e)
        ws.append(w)
        bs.append(b)
        maps.append(random_map((n, k), 9610 + e))
    whats = [what0] + [_what(ws[e], maps[e]) for e in (1, 2)]
    for e in (1, 2):
        _grid_preconditions(x, whats[e], bs[e].astype(np.float64))
    batch = packed.batch_of(packed.pack_batch(torch.from_numpy(np.stack(ws)).cuda(), np.stack(maps), backend="hip"))
    rows = (0, 100, 100, 300)                        # groups of 100, 0 and 200 rows: rows 255 and 256 are of the last, chunk by chunk
    xv = _rows_view(big, torch.bfloat16, T, k, PITCH_16)
    xv.copy_(_x_dev(x))
    want = np.zeros((T, n))
    for e in range(3):
        r0, r1 = rows[e], rows[e + 1]
        want[r0:r1] = _want_y(x[r0:r1], whats[e], bs[e], True)
    bd = torch.from_numpy(np.stack(bs)).cuda()
    for split in (1, 2):
        y = hb.packed_linear_skinny_grouped(xv, torch.tensor(rows, dtype=torch.int32, device="cuda"), batch.arena, batch.maps_dev, batch.offsets_dev,
                                            batch.bases_dev, 3, n, bias=bd, split=split).cpu().numpy().astype(np.float64)
        _same_rows(y, want, ("grouped", split, "X at a far pitch"))


def test_batched_matrices_past_element_2_31(big):
    count, rows, cols = 5, 70, 100
    x = np.stack([gen("heavy_bf16", 9700 + i, (rows, cols)) for i in range(count)])
    maps = np.stack([random_map((rows, cols), 9710 + i) for i in range(count)])
    buf = big.get(2 * ((count - 1) * MATRIX_STRIDE + rows * cols) + 64)
    view = torch.as_strided(buf.view(torch.bfloat16), (count, rows, cols), (MATRIX_STRIDE, cols, 1))
    assert 4 * MATRIX_STRIDE > 2 ** 31 and view[4].data_ptr() - buf.data_ptr() > 2 ** 32
    view.copy_(torch.from_numpy(x).to(torch.bfloat16).cuda())
    pts = packed.pack_batch(view, maps, backend="hip")
    want = np.stack([expected_bits(x[i], maps[i]) for i in range(count)])
    near = packed.unpack_batch(pts, backend="hip").cpu().numpy().view(np.uint32)
    for i in range(count):
        assert np.array_equal(near[i], want[i]), ("pack read a wrong matrix", i, np.argwhere(near[i] != want[i])[:4])
        assert np.array_equal(pts[i].data.cpu().numpy(), packed.pack(x[i], maps[i], backend="emulation").data), i
    view.fill_(-7.0)
    b = packed.batch_of(pts)
    hb.unpack_tiles_batched(b.arena, b.maps_dev, b.offsets_dev, b.bases_dev, count, rows, cols, torch.bfloat16, out=view)
    far = view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << np.uint32(16)
    for i in range(count):
        assert np.array_equal(far[i], want[i]), ("unpack wrote a wrong matrix", i, np.argwhere(far[i] != want[i])[:4])


@pytest.mark.parametrize("entry", ["block", "wide"])
def test_float32_y_row_past_element_2_31(big, entry):
    """257 rows at a pitch of 2²³ + 8 float32: row 256 starts past element 2³¹ (8.0 GiB, the module's largest buffer; runs last)."""
    assert (256 * PITCH_16 + 200) * 4 + 64 < 9 * 2 ** 30
    _y_at_a_far_pitch(big, entry, torch.float32, PITCH_16, 257)
