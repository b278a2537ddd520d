"""The bf16 stats kernel's tail-class redo (csrc/mtq_fast.hip): a group that holds an element more than 14 binades below its maximum
(or a zero) has Σx, Σx² and Σ|x−y| formed again as S_main + S_tail, the offending lanes' groups one after the other with the tile's 16
lanes sharing the work.  Planted inputs — bf16 magnitudes in [0.5, 2) with tail elements, zeros and extremes at chosen places — must
give the oracle's records bit for bit through every route the kernel serves: whole records under every mask, the partial records of the
streamed search (`<3,1>`) and the listed completion of exactly the planted tiles.

The shapes are the smallest the kernel serves: one 32x128 unit, 64x256, a batch of 3 x (32x384), and 32x2560 (20 units: more than a
wave's 8, an odd count after retirement).  The cases are built, and checked for what they claim to hold, on the CPU at import."""
import numpy as np
import pytest

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb

NAMES = ["bf16", "bfp8", "bfp4", "bfp2"]
SHAPES = {"one_unit": (1, 32, 128), "64x256": (1, 64, 256), "batch3": (3, 32, 384), "20_units": (1, 32, 2560)}
TOP = np.float32(1.9921875)               # the largest bf16 of the binade [1, 2): rounds up and saturates in every BFP format
A15 = np.float32(1.9921875 * 2.0 ** -15)  # with 2^-70 between +A15 and -A15 the float64 sum depends on the order


def _bf16(x):
    """float32 values truncated to bf16 precision (what the generator draws; the planted constants are bf16 already)"""
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _base(shape, seed):
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.5, 1.99, size=shape).astype(np.float32)
    return _bf16(np.where(rng.random(shape) < 0.5, -mag, mag))


def _places(shape):
    """(tensor, tile row, unit column) places a case is planted at: the first unit and the last one (one place in a one-unit tensor)"""
    count, rows, cols = shape
    first, last = (0, 0, 0), (count - 1, rows // 32 - 1, cols // 128 - 1)
    return [first] if last == first else [first, last]


class Plant:
    """One case: the tensor and the tiles (tensor, tile row, tile column) something was planted in."""

    def __init__(self, shape, seed):
        self.x = _base(shape, seed)
        self.tiles = set()
        self.out_of_range = set()
        self.b = self.tr = self.u = 0

    def at(self, b, tr, u):
        self.b, self.tr, self.u = b, tr, u
        return self

    def group(self, tile, row, half, unit=None):
        """view of the 16 elements of a group: tile 0..3 of the unit, row 0..31 of the tile (lane row // 2), half 0 / 1 of the tile's columns"""
        unit = self.u if unit is None else unit
        self.tiles.add((self.b, self.tr, unit * 4 + tile))
        c = unit * 128 + tile * 32 + half * 16
        return self.x[self.b, self.tr * 32 + row, c:c + 16]


def _single(p):
    # one tail element per group: each of the four group positions of a lane (row parity x column half), at the first AND at the last element index
    for k, (par, half) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for row, idx in ((2 * (3 + k) + par, 0), (2 * (9 + k) + par, 15)):
            p.group(k % 4, row, half)[idx] = np.float32(1.5 * 2.0 ** -20) * (-1 if (k + idx) & 2 else 1)
    g = p.group(1, 31, 1)
    g[15] = np.float32(-1.25 * 2.0 ** -18)
    g = p.group(1, 0, 0)
    g[0] = np.float32(1.75 * 2.0 ** -30)


def _order(p):
    # two and three tail elements whose float64 sum depends on the order, under a maximum in [1, 2)
    g = p.group(2, 10, 0)
    g[:] = _bf16(np.linspace(1.0, 1.9, 16))
    g[3], g[7], g[12] = A15, np.float32(2.0 ** -70), -A15
    g = p.group(2, 11, 1)
    g[:] = _bf16(np.linspace(-1.9, -1.0, 16))
    g[14], g[15] = np.float32(2.0 ** -70), A15
    g = p.group(0, 21, 0)
    g[0], g[1], g[2] = -A15, A15, np.float32(-(2.0 ** -70))


def _fifteen(p):
    g = p.group(3, 17, 1)
    g[:] = _bf16([(-1) ** i * (1.0 + i / 16.0) * 2.0 ** -(15 + 2 * i) for i in range(16)])
    g[6] = np.float32(1.5)
    g = p.group(0, 0, 0)
    g[:] = _bf16([(1.0 + i / 32.0) * 2.0 ** -15 for i in range(16)])
    g[15] = np.float32(-1.0)


def _tile16(p):
    for j in range(16):
        p.group(1, 2 * j + (j & 1), (j >> 1) & 1)[j] = np.float32((1.0 + j / 16.0) * 2.0 ** -(16 + j)) * (-1 if j % 3 == 0 else 1)


def _wave64(p):
    for lane in range(64):
        t, j = lane >> 4, lane & 15
        p.group(t, 2 * j + ((lane >> 1) & 1), lane & 1)[(5 * lane) % 16] = np.float32((1.0 + j / 16.0) * 2.0 ** -(15 + t)) * (-1 if lane % 5 == 0 else 1)


def _wave64_same(p):
    # every lane's tail element in the SAME group position (even row, first half): one entry of the redo with all 64 lanes as owners
    for lane in range(64):
        t, j = lane >> 4, lane & 15
        p.group(t, 2 * j, 0)[(7 * lane + 3) % 16] = np.float32((1.0 + j / 16.0) * 2.0 ** -(16 + t)) * (-1 if lane % 3 == 0 else 1)
    p.group(2, 5, 1)[:] = _bf16([(1.0 + i / 16.0) * 2.0 ** -(15 + i) for i in range(16)])   # ... and a group of fifteen in another position
    p.group(2, 5, 1)[8] = np.float32(-1.0)


def _two_tiles(p):
    p.group(0, 4, 0)[9] = np.float32(1.5 * 2.0 ** -16)
    p.group(3, 29, 1)[2] = np.float32(-1.5 * 2.0 ** -16)
    p.group(3, 28, 1)[2] = np.float32(1.0 * 2.0 ** -126)


def _zeros(p):
    p.group(0, 6, 1)[5] = np.float32(0.0)       # a lone +0: the zero-only entry
    p.group(2, 13, 0)[15] = np.float32(-0.0)    # a lone -0
    g = p.group(1, 20, 0)                       # a zero together with a tail element
    g[1], g[2] = np.float32(-0.0), np.float32(-1.5 * 2.0 ** -22)
    g = p.group(1, 21, 0)
    g[0], g[15] = np.float32(1.0 * 2.0 ** -15), np.float32(0.0)


def _saturating(p):
    g = p.group(2, 2, 1)
    g[4], g[5] = TOP, np.float32(1.5 * 2.0 ** -15)
    g = p.group(2, 3, 0)
    g[:] = -TOP
    g[11] = np.float32(-1.9921875 * 2.0 ** -15)
    g = p.group(0, 30, 1)
    g[0], g[15] = np.float32(1.25 * 2.0 ** -40), -TOP


def _mixed(p):
    # a unit that also holds an out-of-range tile (E = 67: the literal fix-up takes it) and an all-zero group
    g = p.group(3, 8, 0)
    g[:] = _bf16(g * np.float32(2.0 ** -60))
    p.out_of_range.add((p.b, p.tr, p.u * 4 + 3))
    p.group(1, 12, 1)[:] = np.float32(0.0)
    p.group(1, 13, 1)[7] = np.float32(1.5 * 2.0 ** -17)
    p.group(0, 1, 0)[0] = np.float32(-1.5 * 2.0 ** -19)


CASES = {"single": _single, "order": _order, "fifteen": _fifteen, "tile16": _tile16, "wave64": _wave64, "wave64_same": _wave64_same, "two_tiles": _two_tiles,
         "zeros": _zeros, "saturating": _saturating, "mixed": _mixed}


def _groups(x):
    return x.reshape(x.shape[0], x.shape[1], x.shape[2] // 16, 16)


def _tail_groups(x):
    """groups that hold a tail-class element by the oracle's definition: 0 <= |x| < 2^(E-127-14) in a group that is not all-zero"""
    g = np.abs(_groups(x)).astype(np.float64)
    e = (g.max(axis=-1).astype(np.float32).view(np.uint32) >> 23).astype(np.int64)
    thr = np.ldexp(1.0, e - 141)
    return ((g < thr[..., None]).any(axis=-1)) & (g.max(axis=-1) > 0)


def _tile_exponents_ok(x, b, tr, tc):
    g = np.abs(_groups(x)[b, 32 * tr:32 * tr + 32, 2 * tc:2 * tc + 2]).astype(np.float32)
    e = (g.max(axis=-1).view(np.uint32) >> 23).astype(np.int64)
    return bool(np.all(((e >= 80) & (e <= 180)) | (g.max(axis=-1) == 0)) and np.isfinite(g).all())


def _build(shape_name, case):
    shape = SHAPES[shape_name]
    p = Plant(shape, seed=1000 + 17 * sorted(SHAPES).index(shape_name) + sorted(CASES).index(case))
    for b, tr, u in _places(shape):
        CASES[case](p.at(b, tr, u))
    # the listed route wants a list whose length is no multiple of 4: one more tail element in a tile nothing was planted in, where there is one
    count, rows, cols = shape
    spare = [(b, tr, tc) for b in range(count) for tr in range(rows // 32) for tc in range(cols // 32) if (b, tr, tc) not in p.tiles]
    if len(p.tiles) % 4 == 0 and spare:
        b, tr, tc = spare[len(spare) // 2]
        p.at(b, tr, tc // 4).group(tc % 4, 9, 1)[4] = np.float32(2.0 ** -33)
    return p


PLANTS = {(s, c): _build(s, c) for s in SHAPES for c in CASES}
# what every case claims to hold, checked before anything touches the GPU
for (_s, _c), _p in PLANTS.items():
    assert np.array_equal(_p.x, _bf16(_p.x)), (_s, _c)
    _tg = _tail_groups(_p.x)
    assert _tg.any(), (_s, _c, "no tail-class group")
    # every tail-class group lies in a planted tile (the base holds none), and every planted tile holds one or is the out-of-range one
    for _b, _r, _g in zip(*np.nonzero(_tg)):
        assert (int(_b), int(_r) // 32, int(_g) // 2) in _p.tiles, (_s, _c)
    for _t in _p.tiles:
        assert _tile_exponents_ok(_p.x, *_t) != (_t in _p.out_of_range), (_s, _c, _t)
    assert bool(_p.out_of_range) == (_c == "mixed"), (_s, _c)


def _want(x, formats):
    return np.stack([orc.tile_stats(x[b], formats) for b in range(x.shape[0])])


def _columns(layout, full, sums=0, err=0):
    cols, slot = [], 0
    for f in range(4):
        if not layout & (1 << f):
            continue
        o = 2 + 5 * slot
        if full & (1 << f):
            cols += list(range(o, o + 5))
        elif sums & (1 << f):
            cols += list(range(o, o + 3))
        elif err & (1 << f):
            cols += [o + 3, o + 4]
        slot += 1
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_tail_class_records_bit_exact(shape_name, case):
    import torch

    p = PLANTS[(shape_name, case)]
    x = p.x
    count, rows, cols = x.shape
    tiles = (rows // 32) * (cols // 32)
    xd = torch.from_numpy(x).to(torch.bfloat16).cuda()
    assert np.array_equal(xd.float().cpu().numpy().view(np.uint32), x.view(np.uint32))

    # whole records under every mask the fast kernel serves (at least one BFP format, bf16 slot or not)
    for mask in range(2, 16):
        if not mask & 0xE:
            continue
        fm = [n for i, n in enumerate(NAMES) if mask & (1 << i)]
        want = _want(x, fm)
        got = np.stack([hb.tile_stats(xd[b], mask).cpu().numpy() for b in range(count)])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (shape_name, case, hex(mask))

    # the streamed search's partial records (<3,1>), then the listed completion of exactly the planted tiles (<4,6>); the same on the
    # two-format layout (<2,0> and the listed <2,3>)
    ids = np.array(sorted(b * tiles + tr * (cols // 32) + tc for b, tr, tc in p.tiles), dtype=np.int32)
    assert ids.size % 4 != 0 or ids.size == count * tiles   # (every tile of the tensor planted: nothing to add)
    sel = torch.from_numpy(ids.astype(np.int64)).cuda()
    for layout, full, sums, lfull, lerr in ((0xE, 0x2, 0x4, 0x8, 0x4), (0x6, 0x0, 0x2, 0x4, 0x2)):
        fm = [n for i, n in enumerate(NAMES) if layout & (1 << i)]
        want = torch.from_numpy(_want(x, fm)).cuda().view(count * tiles, -1)
        got = hb.tile_stats_partial(xd, layout, full, sums)
        pcols = [0, 1] + _columns(layout, full, sums)
        assert torch.equal(got.view(count * tiles, -1)[:, pcols].view(torch.int64), want[:, pcols].view(torch.int64)), (shape_name, case, hex(layout), "partial")
        listed = torch.zeros((count * tiles,), dtype=torch.int32, device="cuda")
        listed[: ids.size] = torch.from_numpy(ids).cuda()
        nl = torch.tensor([ids.size], dtype=torch.int32, device="cuda")
        scratch = torch.empty((count * tiles + 1,), dtype=torch.int32, device="cuda")
        work = got.clone()
        hb.tile_stats_listed(xd, layout, lfull, lerr, listed, nl, work, scratch=scratch)
        lcols = _columns(layout, lfull, err=lerr)
        flat = work.view(count * tiles, -1)
        assert torch.equal(flat[sel][:, lcols].view(torch.int64), want[sel][:, lcols].view(torch.int64)), (shape_name, case, hex(layout), "listed")
        rest = torch.ones(count * tiles, dtype=torch.bool, device="cuda")
        rest[sel] = False
        assert torch.equal(flat[rest].view(torch.int64), got.view(count * tiles, -1)[rest].view(torch.int64))   # unlisted tiles untouched
