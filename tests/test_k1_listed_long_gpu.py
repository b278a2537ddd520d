"""GPU: the listed K1 evaluation (mtq_tile_stats_listed) on lists long enough that a wave takes a second and a third item.

Both listed kernels size their grid by the list's CAPACITY, cap it at what fills the chip once, and let every wave stride through the
list with the next item's rows in flight (tile_stats_listed in csrc/mtq_direct.hip: `nxt` / `gt_next`; the LISTED form of
tile_stats_bf16_rolled in csrc/mtq_fast.hip: `here` / `next`).  The lists of tests/k1_claim_cases.py listed_cases() and of
tests/test_hip_kernels.py hold at most 288 tiles, sorted: one item per wave.  Here every list is at least 2.5 rounds of its kernel:

    direct form        12 x CUs tiles a round        (cus * MTQ_DIRECT_WAVES_PER_SIMD * 4 waves, one tile each)
    fast form          16 x lw x CUs tiles a round   (cus * lw * 4 waves of four tiles; lw = MTQ_LISTED_WAVES if positive, else 4)
    handed-back tiles  128 tiles a round             (the W = 1 launch over the tiles the fast form could not take: 128 blocks of one wave)

in ascending, descending and shuffled order (phase 1 of the search appends with an atomic: production lists are not sorted), with all
tiles and with a length of 4k + 1, plus: a claimed length above the capacity, five tiles in a large capacity, and a list made of
nothing but tiles the exact route hands back.

Inputs are tests/k1_claim_cases.py uniform_case batches (three distinct tensors through the oracle, repeated in a shuffled order; each
carries a spoiled site, so a bf16 list of all tiles holds several hundred hand-backs).  Every launch: mtq_tile_stats_partial into
sentinel-filled records; the listed tiles' listed columns overwritten with the sentinel (the literal fix-up of the partial launch wrote
WHOLE records for the spoiled tiles: a listed kernel that skipped them would otherwise pass); mtq_tile_stats_listed; then the listed
tiles' listed columns hold the oracle's bits, and every other double of every record is what it was before the call.  The records of
both launches lie between GUARD records of the sentinel, which must still hold it afterwards.
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from tests import k1_claim_cases as kc

pytestmark = pytest.mark.gpu

GUARD = 64           # sentinel records before and after the records of every launch
BACK_ROUND = 128      # mtq_direct.hip mtq_tile_stats_listed: `grid = dim3(grid.x < 128u ? grid.x : 128u)` blocks of W = 1 wave, one tile a wave


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _direct_round() -> int:
    """mtq_direct.hip mtq_tile_stats_listed: `max_blocks = cus * MTQ_DIRECT_WAVES_PER_SIMD * 4 / kDirectWaves` blocks of kDirectWaves
    waves (3 waves per SIMD, 4 SIMDs), one tile per wave and round."""
    return 12 * _cus()


def _fast_round() -> int:
    """mtq_fast.hip mtq_launch_tile_stats_bf16_listed: `max_blocks = cus * (lw > 0 ? lw : 4) * 4 / kFastWaves` blocks of kFastWaves
    waves, a unit of four list entries per wave and round; lw = atoi(MTQ_LISTED_WAVES)."""
    return 16 * _listed_waves(os.environ.get("MTQ_LISTED_WAVES")) * _cus()


def _listed_waves(text) -> int:
    """The library's `lw > 0 ? lw : 4` with lw = atoi(text): leading white space, a sign, then the leading digits; 0 without any."""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)([0-9]+)", text or "")
    lw = int(m.group(2)) * (-1 if m.group(1) == "-" else 1) if m else 0
    return lw if lw > 0 else 4


assert [_listed_waves(t) for t in (None, "", "0", "-3", "x", "4x", " 8abc", "+2", "1")] == [4, 4, 4, 4, 4, 4, 8, 2, 1]


# name: (kernel of the case, layout, partial full, partial sums, listed full, listed err, scratch given, tiles per round)
ROUTES = {
    "fast-e84": (kc.BF16, 0xE, 0x2, 0x4, 0x8, 0x4, True, _fast_round),        # the two mask pairs the fast form serves
    "fast-642": (kc.BF16, 0x6, 0x0, 0x2, 0x4, 0x2, True, _fast_round),
    "direct-bf16": (kc.BF16, 0xE, 0x6, 0x0, 0x8, 0x0, False, _direct_round),  # a pair the fast form does not serve, and no scratch
    "direct-float32": (kc.DIRECT, 0xE, 0x2, 0x4, 0x8, 0x4, False, _direct_round),
}


@functools.lru_cache(maxsize=None)
def _case(kind: int) -> kc.Case:
    """bf16: tensors of 256 x 512 (128 tiles); float32: 187 x 247 (48 tiles, ragged both ways); as many as 2.5 rounds and 8 tiles take."""
    a, b, per, rnd = (8, 4, 128, _fast_round()) if kind == kc.BF16 else (6, 8, 48, _direct_round())
    count = max(3, -(-(5 * rnd // 2 + 8) // per))
    case = kc.uniform_case(kind, count * a * b, 31 + kind, force=(count, a, b, 3))
    assert case.idx.numel() == count * per >= 2.5 * rnd + 8
    assert tuple(case.x.shape) == ((count, 256, 512) if kind == kc.BF16 else (count, 187, 247))
    return case


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _case.cache_clear()
    _partial.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _partial(kind: int, layout: int, pfull: int, psums: int):
    """(the partial launch's records [T, rec] as int64 bits, the oracle's records in that layout) of _case(kind); never written to."""
    case = _case(kind)
    count = case.x.shape[0]
    T, rec = case.idx.numel(), hb.record_doubles(layout)
    buf = kc.sentinel_filled((GUARD + T + GUARD, rec))
    got = buf[GUARD:GUARD + T].view(count, T // count, rec)
    assert got.data_ptr() == buf[GUARD].data_ptr()
    hb.tile_stats_partial(case.x, layout, pfull, psums, out=got)
    _guards_intact(buf.view(torch.int64), T, "the partial launch")
    fails = case.check(got, layout, "partial", cols=kc.promised_columns(layout, pfull, psums))
    assert not fails, fails
    want = case.full[:, kc.layout_columns(layout)][case.idx]
    return got.reshape(T, rec).view(torch.int64).clone(), want


def _guards_intact(bits: torch.Tensor, T: int, what: str) -> None:
    """bits: [GUARD + T + GUARD, rec] int64; the records before and after the launch's own still hold the sentinel."""
    guards = torch.cat([bits[:GUARD], bits[GUARD + T:]])
    assert guards.shape[0] == 2 * GUARD
    hit = torch.nonzero((guards != kc.SENTINEL).any(1))[:, 0]
    assert hit.numel() == 0, f"{what} wrote {hit.numel()} guard records (before the first record: {int((hit < GUARD).sum())}, behind the last: {int((hit >= GUARD).sum())})"


def _ordered(ids: np.ndarray, order: str) -> np.ndarray:
    if order == "ascending":
        return np.sort(ids)
    if order == "descending":
        return np.sort(ids)[::-1].copy()
    assert order == "shuffled"
    out = np.random.default_rng(99).permutation(np.sort(ids))
    assert np.any(np.diff(out) < 0) and np.any(np.diff(out) > 0)
    return out


def _complete(route: str, ids: np.ndarray, capacity=None, claimed=None) -> None:
    """One listed launch over the tiles `ids` (in that order) after the partial launch of `route`, checked as the module says.
    capacity: entries of the `listed` tensor (default: every tile; entries behind the list name the OTHER tiles, so a kernel that
    reads past the list completes records it must not touch); claimed: what *n_listed says (default: len(ids))."""
    kind, layout, pfull, psums, lfull, lerr, with_scratch, _rnd = ROUTES[route]
    case = _case(kind)
    base, want = _partial(kind, layout, pfull, psums)
    T, rec = base.shape
    n = int(ids.size)
    capacity = T if capacity is None else capacity
    assert len(set(ids.tolist())) == n <= capacity <= T and 0 <= ids.min() and ids.max() < T
    others = np.setdiff1d(np.arange(T), ids)
    store = torch.from_numpy(np.concatenate([ids, others]).astype(np.int32)).cuda()      # the whole buffer is valid tile numbers
    listed = store[:capacity]
    nl = torch.tensor([n if claimed is None else claimed], dtype=torch.int32, device="cuda")
    scratch = torch.empty((capacity + 1,), dtype=torch.int32, device="cuda") if with_scratch else None
    sel = torch.from_numpy(ids.astype(np.int64)).cuda()
    lcols = torch.tensor(kc.promised_columns(layout, lfull, err=lerr), device="cuda")
    framed = kc.sentinel_filled((GUARD + T + GUARD, rec)).view(torch.int64)
    work = framed[GUARD:GUARD + T]                                                      # the launch's records, between guards
    work.copy_(base)
    work[sel[:, None], lcols[None, :]] = kc.SENTINEL
    expect = work.clone()
    expect[sel[:, None], lcols[None, :]] = want[sel[:, None], lcols[None, :]]
    assert not bool((expect[sel][:, lcols] == kc.SENTINEL).any())
    count = case.x.shape[0]
    stats = work.view(torch.float64).view(count, T // count, rec)
    assert stats.data_ptr() == framed[GUARD].data_ptr()
    hb.tile_stats_listed(case.x, layout, lfull, lerr, listed, nl, stats, scratch=scratch)
    _guards_intact(framed, T, f"{route}, {n} of {T} tiles: the listed launch")
    left = (work[sel][:, lcols] == kc.SENTINEL).any(1)
    wrong = (work != expect).any(1)
    if bool(left.any()) or bool(wrong.any()):
        pos = torch.nonzero(left)[:, 0].cpu().numpy()
        is_listed = torch.zeros(T, dtype=torch.bool, device="cuda")
        is_listed[sel] = True
        wl, wo = torch.nonzero(wrong & is_listed)[:, 0].cpu().numpy(), torch.nonzero(wrong & ~is_listed)[:, 0].cpu().numpy()
        where = np.flatnonzero(np.isin(ids, wl))
        pytest.fail(f"{route}, {n} of {T} tiles (capacity {capacity}, claimed {int(nl[0])}): {pos.size} listed tiles not completed (list positions "
                    f"{pos[:8].tolist()}); {wl.size} listed records differ from the oracle (list positions {where[:8].tolist()}, handed back: "
                    f"{int(case.bad[torch.from_numpy(wl).cuda()].sum()) if wl.size else 0}); {wo.size} records outside the list changed (tiles {wo[:8].tolist()})")


def _subset(T: int, n: int) -> np.ndarray:
    return np.random.default_rng(7).choice(T, size=n, replace=False)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_listed_lists_of_more_than_two_rounds(route, order):
    kind, with_scratch, rnd = ROUTES[route][0], ROUTES[route][6], ROUTES[route][7]()
    case = _case(kind)
    T = case.idx.numel()
    short = -(-5 * rnd // 2)
    short += (1 - short) % 4                                                        # the first length of 4k + 1 at or above 2.5 rounds
    assert short % 4 == 1 and 2.5 * rnd <= short < T
    bad = case.bad.cpu().numpy()
    for ids in (_ordered(np.arange(T), order), _ordered(_subset(T, short), order)):
        assert ids.size >= 2.5 * rnd                                                 # a condition on the test: every wave takes a third item
        if with_scratch:
            assert int(bad[ids].sum()) >= 2.5 * BACK_ROUND, int(bad[ids].sum())      # … and so does every wave of the handed-back launch
        _complete(route, ids)


@pytest.mark.parametrize("route", list(ROUTES))
def test_listed_claimed_length_above_capacity(route):
    """*n_listed = n + 4097 with a `listed` tensor of exactly n entries: the first n entries are completed and nothing else changes
    (the tensor is a view of a longer one whose next entries name other tiles: a kernel that read on would write their records)."""
    rnd = ROUTES[route][7]()
    T = _case(ROUTES[route][0]).idx.numel()
    n = -(-5 * rnd // 2)
    n += (1 - n) % 4
    assert n % 4 == 1 and 2.5 * rnd <= n < T - 4
    _complete(route, _ordered(_subset(T, n), "shuffled"), capacity=n, claimed=n + 4097)


@pytest.mark.parametrize("route", list(ROUTES))
def test_listed_short_list_in_large_capacity(route):
    """Five tiles (one of them handed back) in a `listed` tensor of every tile: most waves find nothing."""
    case = _case(ROUTES[route][0])
    T = case.idx.numel()
    bad = np.flatnonzero(case.bad.cpu().numpy())
    ids = np.array([T - 1, 5, int(bad[len(bad) // 2]), T // 2 + 1, 130], dtype=np.int64)
    assert len(set(ids.tolist())) == 5 and T >= 2.5 * ROUTES[route][7]()
    _complete(route, ids)


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("route", ["fast-e84", "fast-642"])
def test_listed_list_of_handed_back_tiles_only(route, order):
    """Every list entry is a tile the exact route cannot take: the fast form completes nothing, the W = 1 launch strides through more
    than 2.5 x 128 of them."""
    case = _case(kc.BF16)
    bad = np.flatnonzero(case.bad.cpu().numpy())
    assert bad.size > BACK_ROUND and bad.size >= 2.5 * BACK_ROUND, bad.size
    _complete(route, _ordered(bad, order))
