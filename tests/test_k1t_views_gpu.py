"""GPU: K1T (mtq_tile_stats_transposed, csrc/mtq_transpose.hip) where it is used and was never tested: on batches that are VIEWS (rows
longer than the matrix, a first element anywhere in a buffer, a matrix stride with slack), with tiles for the literal redo in matrices
other than the first, with more flagged records than one round of the redo's grid takes, and with a matrix past element 2^31.

Every expectation is bit equality with the oracle on Xᵀ, orc.tile_stats(np.ascontiguousarray(x.T), formats); there is no tolerance.
Every launch writes into records filled with tests/k1_claim_cases.py's SENTINEL, GUARD records of it before and after the launch's
own: afterwards no double of the launch's records holds the pattern, the guards still do, and every record has the oracle's bits.

  * views: six shapes x bf16 / float32 x ld - cols in {0, 1, 2, 8} x first element 0..3 x stride slack {0, 1, 6}, count 3, built with
    torch.as_strided over one flat buffer that is NaN wherever no matrix lies, and a second time over 3.0.  K1T pads with +0.0, so an
    element read outside a matrix (the neighbour ColPair::load must not take when cols is odd and pairs are allowed) changes a record:
    the redo's stray read through the NaN, K1T's own through the 3.0 (a NaN it reads flags the tile, and the redo, reading within
    bounds, repairs the record: a wrong load would go unnoticed).  pair_ok is worked out here as the entry point does (pointer, ld,
    stride); the tests assert they saw both values, and pair_ok = 1 with an odd cols;
  * the redo in a batch: the same views with matrices 1 and 2 carrying +Inf, NaN, a denormal-only column group, a group scaled by
    2^-100 and an element of 2^60 in tiles with cb > 0 and rb > 0 where the shape has one; matrix 0 and every other tile stay on the
    exact route (checked with the rule of csrc/mtq_direct.hpp: a group is handed over when its largest exponent field is outside
    [80, 180] and it is not all zero).  Masks 0xF, 0xA, 0x4: three different record lengths and slot offsets;
  * the redo's rounds: its grid is at most 512 blocks of 4 waves of 64 records = 131 072 records a round.  65 786 matrices of 33 x 33
    (four ragged Xᵀ tiles each: 263 144 records, 2 rounds and 1000 records) gathered on the device from a pool of 8 that went through
    the oracle; flagged records at 0, 131 071, 131 072, 262 144, the last one and inside each of the three rounds;
  * far: two 40 x 72 bf16 matrices 2^31 + 2 and 2^31 + 3 elements apart in one torch.empty buffer of 4.3 GB that is never filled, NaN
    in a frame around each; matrix 1 holds a flagged tile, so K1T and the redo both read at the far base.  torch.cuda.OutOfMemoryError
    from that allocation is the module's only skip.

test_k1t_view_parametrisation_has_both_pair_modes and test_k1t_redo_values_hold_every_kind touch no device: they are assertions about
what the GPU tests beside them are given (both pair_ok values, every kind of flagged tile), kept here so that they run, and fail, with them.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from tests import k1_claim_cases as kc
from tests.inputs import gen

pytestmark = pytest.mark.gpu

COUNT = 3
GUARD = 64                                            # sentinel records before and after a launch's own
FRAME = 4096                                          # NaN elements before the first and after the last matrix of a buffer (even)
SHAPES = [(33, 47), (40, 130), (64, 128), (1, 257), (70, 1), (37, 96)]
ALL_MASKS = {(33, 47), (40, 130)}                     # the shapes that run all 15 masks
FEW_MASKS = (0xF, 0x6, 0x9)
REDO_MASKS = (0xF, 0xA, 0x4)
PADS, OFFSETS, SLACKS = (0, 1, 2, 8), (0, 1, 2, 3), (0, 1, 6)
VIEWS = list(itertools.product(PADS, OFFSETS, SLACKS))
# What lies outside the matrices.  NaN: a stray read of the literal redo makes its record NaN.  A stray read of K1T's own loads must not be
# NaN, though: a NaN makes the group one the exact route hands over, and the redo, which reads within bounds, would put the record right.
# So every view runs a second time over 3.0, which the exact route takes and which changes Σx of the tile it strays into.
FILLS = (float("nan"), 3.0)
REDO_ROUND = 512 * 4 * 64                             # mtq_tile_stats_transposed: rgrid = min(.., 512) blocks x 4 waves x 64 records


def _dtype(bf16: bool):
    return torch.bfloat16 if bf16 else torch.float32


def _store(vals: np.ndarray, bf16: bool) -> torch.Tensor:
    """vals on the device in that storage type with EXACTLY the oracle's bits: bf16 storage takes the high halves of the (bf16-valued)
    float32 words, since a cast would replace the bits of a NaN."""
    words = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32)
    if not bf16:
        return torch.from_numpy(words.view(np.float32).copy()).cuda()
    assert not np.any(words & np.uint32(0xFFFF))
    return torch.from_numpy((words >> np.uint32(16)).astype(np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _values(rows: int, cols: int, bf16: bool) -> np.ndarray:
    """COUNT finite matrices as float32 values (bf16-valued for bf16 storage)."""
    x = gen("heavy_bf16" if bf16 else "heavy_f32", 7000 + 10 * rows + cols, (COUNT, rows, cols))
    assert np.isfinite(x).all()
    return x


def _flagged(x: np.ndarray) -> set:
    """The Xᵀ tiles of x (rows, cols) that the exact route hands to the literal one, by the rule of csrc/mtq_direct.hpp: a group (16
    consecutive rows of one column of X, zero-padded) whose largest |element| has an exponent field outside [80, 180] and is not 0."""
    rows, cols = x.shape
    th = -(-rows // 32)
    mag = np.zeros((th * 32, cols), dtype=np.uint32)
    mag[:rows] = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    m = mag.reshape(th * 2, 16, cols).max(axis=1)                                    # [row group, column]
    e = m >> np.uint32(23)
    bad = (m != 0) & ((e < 80) | (e > 180))
    return {(c // 32) * th + g // 2 for g, c in zip(*np.nonzero(bad))}


def _oracle_bits(vals: np.ndarray, mask: int) -> torch.Tensor:
    """The oracle's records of every matrix's transpose, [count * tiles, rec] int64 bits on the device."""
    with np.errstate(all="ignore"):
        rec = np.stack([orc.tile_stats(np.ascontiguousarray(v.T), hb.mask_formats(mask)) for v in vals])
    return torch.from_numpy(rec.view(np.int64).reshape(-1, rec.shape[-1])).cuda()


def _pair_ok(view) -> int:
    """mtq_tile_stats_transposed: pair_ok = base pointer % (2 * element size) == 0 && ld % 2 == 0 && (count == 1 || stride_elems % 2 == 0)."""
    _code, count, stride, _rows, _cols, ld = hb._matrix(view)
    return int(view.data_ptr() % (2 * view.element_size()) == 0 and ld % 2 == 0 and (count == 1 or stride % 2 == 0))


def _launch(view, mask: int, want: torch.Tensor):
    """K1T on `view` into sentinel-filled records between guards → (device flags: a record still holds the sentinel, a guard was
    written, a record differs from the oracle; the launch's records as int64 bits)."""
    n, rec = want.shape
    assert rec == hb.record_doubles(mask)
    out = kc.sentinel_filled((GUARD + n + GUARD, rec))
    count = view.shape[0] if view.dim() == 3 else 1
    got = hb.tile_stats_transposed(view, mask, out=out[GUARD:GUARD + n].view(count, n // count, rec))
    assert got.data_ptr() == out[GUARD].data_ptr()
    g = out.view(torch.int64)
    body = g[GUARD:GUARD + n]
    guards = torch.cat([g[:GUARD], g[GUARD + n:]])
    return torch.stack([(body == kc.SENTINEL).any(), (guards != kc.SENTINEL).any(), (body != want).any()]), body


def _batch_view(src: torch.Tensor, pad: int, off: int, slack: int, fill: float):
    """src (count, rows, cols) as a view with ld = cols + pad, the first element `off` elements into the space behind the frame and
    matrices rows * ld + slack apart, over a flat buffer that holds `fill` everywhere else."""
    count, rows, cols = src.shape
    ld = cols + pad
    stride = rows * ld + slack
    buf = torch.full((FRAME + off + (count - 1) * stride + rows * ld + FRAME,), fill, dtype=src.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (count, rows, cols), (stride, ld, 1), FRAME + off)
    view.copy_(src)
    outside = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
    torch.as_strided(outside, (count, rows, cols), (stride, ld, 1), FRAME + off).fill_(False)
    assert int(outside.sum()) == buf.numel() - src.numel()
    assert bool((torch.isnan(buf[outside]) if fill != fill else buf[outside] == fill).all())   # everything outside the matrices is the fill
    return view


def _pair_ok_of(rows: int, cols: int, pad: int, off: int, slack: int) -> int:
    """_pair_ok of _batch_view's view (its buffer is 16-byte aligned and FRAME is even), from the numbers alone."""
    ld = cols + pad
    return int(off % 2 == 0 and ld % 2 == 0 and (rows * ld + slack) % 2 == 0)


def _run_views(vals: np.ndarray, bf16: bool, masks):
    src = _store(vals, bf16)
    assert src.dtype == _dtype(bf16) and src.shape == vals.shape
    want = {mask: _oracle_bits(vals, mask) for mask in masks}
    flags, names, seen = [], [], set()
    for (pad, off, slack), fill in itertools.product(VIEWS, FILLS):
        view = _batch_view(src, pad, off, slack, fill)
        pk = _pair_ok(view)
        assert pk == _pair_ok_of(vals.shape[1], vals.shape[2], pad, off, slack)
        seen.add(pk)
        for mask in masks:
            flags.append(_launch(view, mask, want[mask])[0])
            names.append((pad, off, slack, fill, hex(mask), f"pair_ok={pk}"))
    res = torch.stack(flags).cpu().numpy()
    for col, what in enumerate(("records still hold the sentinel (not computed)", "guard records were written", "records differ from the oracle")):
        bad = [names[i] for i in np.flatnonzero(res[:, col])]
        assert not bad, (what, len(bad), bad[:6])
    assert seen == {0, 1}                             # both load forms ran on this shape; with an odd cols, pair_ok = 1 is the last column's case
    return len(flags)


# ------------------------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "float32"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_k1t_batch_views_equal_oracle(rows, cols, bf16):
    vals = _values(rows, cols, bf16)
    assert all(not _flagged(v) for v in vals)
    masks = tuple(range(1, 16)) if (rows, cols) in ALL_MASKS else FEW_MASKS
    assert _run_views(vals, bf16, masks) == len(VIEWS) * len(FILLS) * len(masks)


def test_k1t_view_parametrisation_has_both_pair_modes():
    """The views above hold pair_ok = 0 and 1 for even and odd cols alike (every launch checks _pair_ok_of against its real pointer):
    pair_ok = 1 with an odd cols is where ColPair::load must leave the pair load to the last column alone."""
    assert len(SHAPES) == 6 and sum(s in ALL_MASKS for s in SHAPES) == 2 and len(VIEWS) == 48
    seen = {(_pair_ok_of(rows, cols, *v), cols % 2) for rows, cols in SHAPES for v in VIEWS}
    assert seen == {(0, 0), (1, 0), (0, 1), (1, 1)}, seen
    for rows, cols in SHAPES:
        assert {_pair_ok_of(rows, cols, *v) for v in VIEWS} == {0, 1}, (rows, cols)


# ------------------------------------------------------------------------------------------------------------------ the redo in a batch
KINDS_1, KINDS_2 = ("inf", "denormal group", "2^60"), ("nan", "group x 2^-100")       # what matrix 1 and matrix 2 carry


def _spoil(x: np.ndarray, cb: int, rb: int, kind: str, k: int, bf16: bool) -> None:
    """Puts one thing the exact route cannot take into Xᵀ tile (cb, rb) of x: X rows 32 rb .., columns 32 cb .. (column chosen by k)."""
    rows, cols = x.shape
    nr, nc = min(32, rows - 32 * rb), min(32, cols - 32 * cb)
    c = 32 * cb + (5 * k + 1) % nc
    r = 32 * rb + (3 + k) % nr
    g0 = 32 * rb + (16 if nr > 16 else 0)                                            # a whole group of column c: rows g0 .. g0 + 15
    if kind == "inf":
        x[r, c] = np.inf
    elif kind == "nan":
        x[r, c] = np.nan
    elif kind == "2^60":
        x[r, c] = 2.0 ** 60
    elif kind == "denormal group":
        x[g0:g0 + 16, c] = np.float32(2.0 ** -130 if bf16 else 1e-40)                   # bf16 has denormals down to 2^-133
    elif kind == "group x 2^-100":
        x[g0:g0 + 16, c] = np.maximum(np.abs(x[g0:g0 + 16, c]), np.float32(2.0 ** -20)) * np.float32(2.0 ** -100)
    else:
        raise ValueError(kind)


def _redo_values(rows: int, cols: int, bf16: bool):
    """_values with the kinds spread over the target tiles of matrices 1 and 2 → (values, [flagged tiles of each matrix], both > 0)."""
    vals = _values(rows, cols, bf16).copy()
    th, tw = -(-rows // 32), -(-cols // 32)                                          # rb < th, cb < tw
    both = th > 1 and tw > 1
    targets = [(cb, rb) for cb in range(tw) for rb in range(th) if (cb > 0 or tw == 1) and (rb > 0 or th == 1) and (cb, rb) != (0, 0)]
    assert targets and len(targets) < th * tw
    want = [set(), set(), set()]
    k = 0
    for i, kinds in ((1, KINDS_1), (2, KINDS_2)):
        for kind in kinds:
            cb, rb = targets[k % len(targets)]
            _spoil(vals[i], cb, rb, kind, k, bf16)
            want[i].add(cb * th + rb)
            k += 1
    return vals, want, both


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "float32"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_k1t_redo_in_batch_views(rows, cols, bf16):
    vals, want, both = _redo_values(rows, cols, bf16)
    assert both == ((rows, cols) not in ((1, 257), (70, 1)))
    assert [_flagged(v) for v in vals] == want and not want[0] and want[1] and want[2]   # exactly the intended tiles are handed over
    th = -(-rows // 32)
    if both:
        assert all(t // th > 0 and t % th > 0 for t in want[1] | want[2])               # cb > 0 and rb > 0
    assert _run_views(vals, bf16, REDO_MASKS) == len(VIEWS) * len(FILLS) * len(REDO_MASKS)


def test_k1t_redo_values_hold_every_kind():
    """Host only: every kind is in the values of both storage types (as an element that survives the later kinds), on four shapes in
    a tile with cb > 0 and rb > 0."""
    for bf16 in (True, False):
        n_both = 0
        for rows, cols in SHAPES:
            vals, want, both = _redo_values(rows, cols, bf16)
            n_both += both
            mag = np.abs(vals[1:])
            assert np.isposinf(vals[1]).any() and np.isnan(vals[2]).any() and (vals[1] == 2.0 ** 60).any(), (rows, cols)
            assert ((mag > 0) & (mag < 2.0 ** -126)).any() and ((mag >= 2.0 ** -126) & (mag < 2.0 ** -100)).any(), (rows, cols)
        assert n_both == 4


# ------------------------------------------------------------------------------------------------------------------ the redo's rounds
def _round_pool(bf16: bool):
    """8 matrices of 33 x 33: four finite ones, and the first of them with tile t = 2 cb + rb of its Xᵀ handed over, t = 0..3."""
    fin = gen("heavy_bf16" if bf16 else "heavy_f32", 8100 + bf16, (4, 33, 33))
    var = np.stack([fin[0]] * 4)
    var[0, 16:32, 5] = np.maximum(np.abs(var[0, 16:32, 5]), np.float32(2.0 ** -20)) * np.float32(2.0 ** -100)   # tile (0, 0): a group x 2^-100
    var[1, 32, 7] = np.inf                                                                                      # tile (0, 1): X row 32
    var[2, 0:16, 32] = np.float32(2.0 ** -130 if bf16 else 1e-40)                                               # tile (1, 0): a denormal-only group
    var[3, 32, 32] = 2.0 ** 60                                                                                  # tile (1, 1): the corner element
    pool = np.concatenate([fin, var])
    assert [_flagged(p) for p in pool] == [set()] * 4 + [{0}, {1}, {2}, {3}]
    return pool


@pytest.mark.parametrize("mask", [0xF, 0xA], ids=hex)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "float32"])
def test_k1t_redo_second_and_third_round(bf16, mask):
    need = 2 * REDO_ROUND + 1000
    count = -(-need // 4)
    total = 4 * count
    assert REDO_ROUND == 131072 and total >= need and count >= 65786
    assert ((total + 63) // 64 + 3) // 4 > 512                                         # the redo's grid is the capped one
    spots = [0, REDO_ROUND - 1, REDO_ROUND, 2 * REDO_ROUND, total - 1, REDO_ROUND // 2 + 3, REDO_ROUND + REDO_ROUND // 3 + 2, 2 * REDO_ROUND + 501]
    assert {s // REDO_ROUND for s in spots} == {0, 1, 2} and len({s // 4 for s in spots}) == len(spots)
    pool = _round_pool(bf16)
    order = np.random.default_rng(17).integers(0, 4, size=count)
    for s in spots:
        order[s // 4] = 4 + s % 4                                                        # the variant whose flagged tile is record s
    flagged = np.flatnonzero(order >= 4) * 4 + (order[order >= 4] - 4)
    assert sorted(flagged.tolist()) == sorted(spots)
    od = torch.from_numpy(order).cuda()
    x = _store(pool, bf16)[od]
    assert tuple(x.shape) == (count, 33, 33) and x.is_contiguous()
    rec = hb.record_doubles(mask)
    want = _oracle_bits(pool, mask).view(8, 4, rec)[od].reshape(total, rec)
    flags, out = _launch(x, mask, want)
    res = flags.cpu().numpy()
    if res.any():                                                                        # name the records: which round?
        bad = torch.nonzero((out != want).any(1))[:, 0].cpu().numpy()
        pytest.fail(f"sentinel left {bool(res[0])}, guards written {bool(res[1])}; {bad.size} records differ, rounds {sorted({int(b) // REDO_ROUND for b in bad})}, first {bad[:8].tolist()}")


# ------------------------------------------------------------------------------------------------------------------ past element 2^31
FAR_ROWS, FAR_COLS, FAR_LD = 40, 72, 74
FAR_STRIDES = (2 ** 31 + 2, 2 ** 31 + 3)
FAR_ELEMS = FRAME + max(FAR_STRIDES) + FAR_ROWS * FAR_LD + FRAME


@pytest.fixture(scope="module")
def far_buffer():
    torch.cuda.empty_cache()
    try:
        buf = torch.empty((FAR_ELEMS,), dtype=torch.bfloat16, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip(f"out of device memory for the {2 * FAR_ELEMS}-byte buffer of the far-address tests (the only permitted skip)")
    yield buf
    del buf
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _far_values():
    vals = gen("heavy_bf16", 8200, (2, FAR_ROWS, FAR_COLS))
    vals[1, 35, 66] = np.inf                                                             # Xᵀ tile (cb, rb) = (2, 1) of matrix 1
    assert [_flagged(v) for v in vals] == [set(), {2 * 2 + 1}]
    return vals


@pytest.mark.parametrize("stride", FAR_STRIDES, ids=["even", "odd"])
def test_k1t_matrix_past_element_2_31(far_buffer, stride):
    vals = _far_values()
    src = _store(vals, True)
    span = FAR_ROWS * FAR_LD
    for first in (FRAME, FRAME + stride):                                                # NaN in a frame around the two matrices only
        far_buffer[first - FRAME:first + span + FRAME].fill_(float("nan"))
    view = torch.as_strided(far_buffer, (2, FAR_ROWS, FAR_COLS), (stride, FAR_LD, 1), FRAME)
    view.copy_(src)
    assert view[1].data_ptr() - far_buffer.data_ptr() > 2 ** 32 and stride > 2 ** 31 and FRAME + stride + span + FRAME <= FAR_ELEMS
    assert torch.equal(view[1].contiguous().view(torch.int16), src[1].view(torch.int16))
    assert _pair_ok(view) == int(stride % 2 == 0)
    for mask in (0xF, 0xA):
        res = _launch(view, mask, _oracle_bits(vals, mask))[0].cpu().numpy()
        assert not res.any(), (hex(mask), stride, dict(zip(("sentinel left", "guards written", "records differ"), res.tolist())))
