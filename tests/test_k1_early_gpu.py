"""The early form of the lazy route's K1 launch (csrc/mtq_fast.hip, EARLY): tiles whose rank lies below the cutoff get, beside what the
partial launch <3,1> writes, the statistics the listed launch <4,6> would add — from the rows the wave already holds.  Checked alone against
a whole-record launch (mask 0xE), records compared as uint64:

  * early tiles: every slot equals the whole record's;
  * other tiles: the slots K1 promises equal it, the left-out slots hold the poison NaN;
  * a tile the exact route cannot take (out-of-range exponent, NaN) is marked whether it is early or not, and the fix-up launch writes its
    whole record: early tiles of that kind need no place on the list;
  * cutoff 0: the bytes of the plain partial launch.

Shapes: one 32x128 unit, a batch of 3 x 64x256, and a strided view of 2 x 96x384 (ld 400, batch stride 40008: no multiple of the matrix).
Rank tables are written here so that the units of a launch hold 0, 1, 2, 3 and 4 early tiles (five tables that rotate the counts over
the units); cutoffs 0, half, exactly the early count, and T.  Every group has a binade of its own (2^-20 .. 2^20) so that the float64
sums round and a wrong order of addition shows.  Planted in the first unit: a tail-class element and an all-zero group (tile 0), a NaN
(tile 1), an all-zero tile (tile 2), a group of exponent 67 (tile 3); in the last unit of a larger shape: a tail-class element in an odd
row's last place beside a group of -0.0."""
import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb

POISON = np.uint64(0x7FF8000000000BAD)
LAYOUT, FULL, SUMS = 0xE, 0x2, 0x4
K1_COLS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]            # Σx, Σx², bfp8's five, bfp4's Σy, Σy², Σxy
LEFT_COLS = [10, 11, 12, 13, 14, 15, 16]            # bfp4's Σ|x−y|, max|x−y|; bfp2's five
SHAPES = {"one_unit": (1, 32, 128), "batch3": (3, 64, 256), "view": (2, 96, 384)}
VIEW_LD, VIEW_STRIDE = 400, 40008


def _bf16(x):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _data(shape, seed):
    count, rows, cols = shape
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.5, 1.99, size=shape).astype(np.float32)
    x = np.where(rng.random(shape) < 0.5, -mag, mag).astype(np.float32)
    scale = np.ldexp(np.float32(1.0), rng.integers(-20, 21, size=(count, rows, cols // 16))).astype(np.float32)
    x = _bf16(x * np.repeat(scale, 16, axis=2))

    def group(b, tr, tc, row, half):
        return x[b, tr * 32 + row, tc * 32 + half * 16: tc * 32 + half * 16 + 16]

    planted = {}
    g = group(0, 0, 0, 5, 1)
    g[3] = np.float32(np.abs(g).max() * 2.0 ** -20)                   # tail class: below max·2^-14
    group(0, 0, 0, 12, 0)[:] = 0.0
    planted["tail+zero_group"] = (0, 0)
    group(0, 0, 1, 9, 1)[7] = np.float32("nan")
    planted["nan"] = (0, 1)
    x[0, 0:32, 64:96] = 0.0
    planted["zero_tile"] = (0, 2)
    g = group(0, 0, 3, 8, 0)
    g[:] = _bf16(np.linspace(1.0, 1.9, 16) * 2.0 ** -60)              # exponent 67: outside [80, 180]
    planted["out_of_range"] = (0, 3)
    if count * rows * cols > 32 * 128:
        b, tr, tc0 = count - 1, rows // 32 - 1, cols // 32 - 4
        g = group(b, tr, tc0, 31, 1)
        g[15] = np.float32(-np.abs(g).max() * 2.0 ** -16)
        group(b, tr, tc0, 30, 0)[:] = np.float32(-0.0)
        planted["tail_last"] = (b, tr * (cols // 32) + tc0)
    return x, planted


def _rank_tables(rows, cols):
    """five (rank, early count) pairs: unit u of table s holds (u + s) % 5 early tiles, ranked 0 .. E-1 in tile order; the others follow"""
    tw, units_w = cols // 32, cols // 128
    T = (rows // 32) * tw
    out = []
    for s in range(5):
        early = np.zeros(T, dtype=bool)
        for tr in range(rows // 32):
            for uc in range(units_w):
                u = tr * units_w + uc
                for i in range((u + s) % 5):
                    early[tr * tw + uc * 4 + (u + s + i) % 4] = True
        rank = np.empty(T, dtype=np.uint32)
        rank[early] = np.arange(int(early.sum()), dtype=np.uint32)
        rank[~early] = np.arange(int(early.sum()), T, dtype=np.uint32)
        out.append((rank, int(early.sum())))
    return out


CASES = {name: _data(shape, 4100 + i) for i, (name, shape) in enumerate(SHAPES.items())}
_REF = {}


def _device(name):
    """→ (the input on the device — a strided view for "view" —, the whole-record launch's records as uint64 [count, tiles, 17])"""
    import torch

    if name not in _REF:
        x, _planted = CASES[name]
        src = torch.from_numpy(x).to(torch.bfloat16).cuda()
        if name == "view":
            count, rows, cols = x.shape
            buf = torch.full((16 + (count - 1) * VIEW_STRIDE + rows * VIEW_LD + 16,), float("nan"), dtype=torch.bfloat16, device="cuda")
            xd = torch.as_strided(buf, (count, rows, cols), (VIEW_STRIDE, VIEW_LD, 1), 16)
            xd.copy_(src)
            assert xd.data_ptr() % 16 == 0 and not xd.is_contiguous() and VIEW_STRIDE % (rows * VIEW_LD) != 0 and VIEW_STRIDE % (rows * cols) != 0
        else:
            xd = src
        whole = hb.tile_stats_batched(src, LAYOUT).cpu().numpy().view(np.uint64)
        _REF[name] = (xd, whole)
    return _REF[name]


def _early_launch(xd, rank, cutoff):
    import torch

    count, rows, cols = xd.shape
    tiles = (rows // 32) * (cols // 32)
    out = torch.full((count, tiles, 17), -1.0, dtype=torch.float64, device="cuda")
    mark = torch.zeros((1,), dtype=torch.int32, device="cuda")
    rk = torch.from_numpy(rank.view(np.int32)).cuda()
    lid = hb.tile_stats_partial_begin_early(xd, LAYOUT, FULL, SUMS, out, mark, rk, cutoff)
    before = out.cpu().numpy().view(np.uint64).copy()
    hb.tile_stats_partial_end(xd, LAYOUT, out, mark, lid)
    return before, out.cpu().numpy().view(np.uint64)


def _check(name, rank, cutoff):
    xd, whole = _device(name)
    x, planted = CASES[name]
    count, rows, cols = x.shape
    tiles = (rows // 32) * (cols // 32)
    before, got = _early_launch(xd, rank, cutoff)
    fixup = np.zeros((count, tiles), dtype=bool)
    for kind in ("nan", "out_of_range"):
        fixup[planted[kind]] = True
    early = np.broadcast_to(rank[None, :] < cutoff, (count, tiles))
    done = early | fixup
    assert np.array_equal(got[done], whole[done]), (name, cutoff, "early and fix-up tiles: every slot")
    assert np.array_equal(got[~done][:, K1_COLS], whole[~done][:, K1_COLS]), (name, cutoff, "other tiles: K1's slots")
    assert (got[~done][:, LEFT_COLS] == POISON).all(), (name, cutoff, "other tiles: the left-out slots are poison")
    # the kernel itself marks a tile it cannot take, early or not, and leaves it to the fix-up
    assert (before[fixup][:, 0] == np.uint64(0x7FF8C0DE5EED0001)).all()
    # ... and has written the early tiles' left-out slots before the fix-up ran
    ok = early & ~fixup
    assert np.array_equal(before[ok], whole[ok])
    return early


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_early_tiles_have_whole_records_and_the_others_poison(name):
    x, planted = CASES[name]
    count, rows, cols = x.shape
    tiles = (rows // 32) * (cols // 32)
    seen = np.zeros((count, tiles), dtype=bool)
    per_unit = set()
    for rank, n_early in _rank_tables(rows, cols):
        e = _check(name, rank, n_early)
        seen |= e
        per_unit |= set(e[0].reshape(rows // 32, cols // 128, 4).sum(axis=2).ravel().tolist())
    if name != "one_unit":
        assert per_unit == {0, 1, 2, 3, 4}
    rank, n_early = _rank_tables(rows, cols)[3]
    _check(name, rank, n_early // 2)
    seen |= _check(name, rank, tiles)                                  # every tile early
    assert all(seen[at] for at in planted.values())                    # each planted input sat inside an early tile


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_cutoff_zero_is_the_plain_partial_launch(name):
    import torch

    xd, _whole = _device(name)
    count, rows, cols = xd.shape
    tiles = (rows // 32) * (cols // 32)
    rank = np.arange(tiles, dtype=np.uint32)
    before, got = _early_launch(xd, rank, 0)
    plain = torch.full((count, tiles, 17), -1.0, dtype=torch.float64, device="cuda")
    mark = torch.zeros((1,), dtype=torch.int32, device="cuda")
    src = xd.contiguous()
    lid = hb.tile_stats_partial_begin(src, LAYOUT, FULL, SUMS, plain, mark)
    assert np.array_equal(before, plain.cpu().numpy().view(np.uint64))
    hb.tile_stats_partial_end(src, LAYOUT, plain, mark, lid)
    assert np.array_equal(got, plain.cpu().numpy().view(np.uint64))


@pytest.mark.gpu
def test_the_early_form_refuses_other_layouts():
    import torch

    xd, _whole = _device("one_unit")
    out = torch.empty((1, 4, 12), dtype=torch.float64, device="cuda")
    mark = torch.zeros((1,), dtype=torch.int32, device="cuda")
    rk = torch.zeros((4,), dtype=torch.int32, device="cuda")
    with pytest.raises(hb.MtqError):
        hb.tile_stats_partial_begin_early(xd, 0x6, 0x0, 0x2, out, mark, rk, 2)


def _reference_rank(seed, tiles, which):
    """np.argsort of the permutation the reference's generator draws for pass `which` + 1 while every tile is a candidate"""
    rng = np.random.default_rng(seed)
    for _ in range(which + 1):
        rng.permutation(tiles)
    return np.argsort(rng.permutation(tiles), kind="stable").astype(np.uint32)


# 4 and 128: one block; 16 384 and 57 344: the bench's and Llama's, many blocks; 262 144 + 333: more tiles than 1024 blocks of 256 threads
@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [4, 128, 16384, 57344, 1024 * 256 + 333])
def test_rank_kernel_is_argsort_of_the_reference_permutation(tiles):
    import torch

    seed = 123 if tiles != 128 else 2**63 + 5
    orders = hb.scan_orders_device(seed, tiles, 2)
    for which in (0, 1):
        out = torch.full((tiles + 3,), 7, dtype=torch.int32, device="cuda")           # three guard entries behind the table
        hb.scan_rank_device(orders, tiles, which, out=out)
        got = out.cpu().numpy().view(np.uint32)
        want = _reference_rank(seed, tiles, which)
        assert np.array_equal(got[:tiles], want), (tiles, which)
        assert np.array_equal(got[:tiles], hb.early_rank_host(seed, tiles, which))
        assert (got[tiles:] == 7).all()


@pytest.mark.gpu
def test_rank_of_an_order_that_was_not_drawn_is_all_ones():
    orders = hb.scan_orders_device(123, 128, 1)
    assert np.array_equal(hb.scan_rank_device(orders, 128, 0).cpu().numpy().view(np.uint32), _reference_rank(123, 128, 0))
    assert (hb.scan_rank_device(orders, 128, 1).cpu().numpy().view(np.uint32) == np.uint32(0xFFFFFFFF)).all()
