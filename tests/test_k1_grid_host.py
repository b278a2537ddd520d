"""CPU-only: the grid K1 launches (csrc/mtq_error.hpp k1_grid, read through mtq_debug_k1_grid) against a Python restatement of the
claim discipline of csrc/mtq_fast.hip / csrc/mtq_direct.hip that shares no code with it:

    blocks b = 0 .. B-1 of W waves each; G = min(B, 64) counters; block b claims from counter b % G, i.e. group g gets the blocks
    g, g + G, ...; the k-th claim on counter g is unit g + k * G; a wave makes at most `quota` claims (no limit when quota is 0).

Every unit is computed exactly when each group's claims reach its last unit: blocks(g) * W * quota >= units(g).  A grid that misses
this leaves units nobody computes - records that keep whatever the buffer held (tests/test_k1_work_claim_gpu.py looks for those on
the device; this test looks at every geometry the device at hand does not have)."""
import numpy as np

from quantization_analysis_amd import hip_backend as hb

GROUPS = 64                                     # csrc/mtq_error.hpp kWorkGroups
WAVES_PER_BLOCK = {hb.K1_BF16: 2, hb.K1_DIRECT: 2}   # csrc/mtq_fast.hip kFastWaves, csrc/mtq_direct.hip kDirectWaves
QUOTA_SCALE = {hb.K1_BF16: 1, hb.K1_DIRECT: 16}      # claims per unit of MTQ_K1_UNITS_PER_WAVE (the direct kernel: 16 tiles)
CUS = (1, 2, 3, 7, 64, 80, 104, 228, 256, 304)
WAVES_PER_SIMD = range(1, 9)
QUOTAS = (0, 1, 2, 8, 16, 128, 1000)
LIMIT = 2**31 - 1


def _borders(cus: int, wps: int, W: int, q: int) -> set:
    """Totals at every regime border of that geometry, from the regimes' definitions (not from the function under test)."""
    mb = cus * wps * 4 // W                     # blocks resident at once
    t = {1, 2, W, W + 1, mb * W - 1, mb * W, mb * W + 1}          # the largest total with a wave per unit, and its neighbours
    if q:
        # the largest total whose quota grid ((ceil(by_quota / 64) + 1) * 64 blocks) is still no larger than the resident grid
        whole = (mb // GROUPS - 1) * GROUPS
        for by_quota in (whole, whole + GROUPS):
            if by_quota > 0:
                t |= {by_quota * W * q - 1, by_quota * W * q, by_quota * W * q + 1}
        for k in (1, 2, 3, 17):                 # one below / above a multiple of 64 x W x quota: a group's last block exactly full
            t |= {k * GROUPS * W * q - 1, k * GROUPS * W * q, k * GROUPS * W * q + 1}
    return {v for v in t if 1 <= v <= LIMIT}


def _check(kind: int, total: int, cus: int, wps: int, upw: int) -> str:
    """Asserts the claim discipline covers every unit on the grid the library reports -> the launch's regime."""
    W, q = WAVES_PER_BLOCK[kind], upw * QUOTA_SCALE[kind]
    blocks, quota, groups = hb.k1_grid(kind, total, cus, wps, upw)
    what = (kind, total, cus, wps, upw, blocks, quota, groups)
    need, mb = -(-total // W), cus * wps * 4 // W
    assert blocks >= 1 and groups == min(blocks, GROUPS), what
    assert quota == (q if q and need > mb else 0), what           # waves retire only where there are more units than resident waves
    if quota == 0:
        assert blocks <= need and blocks == min(need, mb), what   # no block without a first unit
    else:
        assert blocks >= mb, what                                 # the resident grid, or more
    g = np.arange(groups, dtype=np.int64)
    units = np.maximum(0, -(-(total - g) // groups))              # units g, g + G, ... below total
    nblocks = -(-(blocks - g) // groups)                          # blocks g, g + G, ... below blocks
    assert (nblocks >= 1).all(), what
    if quota:
        claims = nblocks * W * quota
        short = np.nonzero(claims < units)[0]
        assert short.size == 0, (what, "units nobody claims in groups", short[:4].tolist())
        # the launcher's stated margin: every group has one block more than its units take at `quota` per wave (a block that finds
        # its queue empty exits at once), so that a change of the rounding cannot eat into coverage unnoticed
        tight = np.nonzero(claims < units + W * quota)[0]
        assert tight.size == 0, (what, "no spare block in groups", tight[:4].tolist())
    if need <= mb:
        assert blocks * W >= total, what                          # a wave for every unit
        return "resident"
    if quota == 0:
        return "persistent"
    return "quota" if blocks == mb else "oversubscribed"


def test_waves_per_block_and_argument_checks():
    for kind, W in WAVES_PER_BLOCK.items():
        assert hb.k1_waves_per_block(kind) == W
    assert hb.k1_grid(hb.K1_BF16, 128 * 128 * 32, 256, 3, 8) == (32832, 8, 64)       # 128 x 4096^2 bf16 on 256 CUs, default switches
    assert hb.k1_grid(hb.K1_BF16, 23552, 256, 3, 8)[0] == 1536 and hb.k1_grid(hb.K1_BF16, 23553, 256, 3, 8)[0] == 1600
    assert hb.k1_grid(hb.K1_DIRECT, 376832, 256, 3, 8)[0] == 1536 and hb.k1_grid(hb.K1_DIRECT, 376833, 256, 3, 8)[0] == 1600
    assert hb.k1_grid(hb.K1_DIRECT, 10**6, 256, -1, 8)[1] == 128
    for bad in ((7, 100, 256, 3, 8), (hb.K1_BF16, 0, 256, 3, 8), (hb.K1_BF16, 100, 0, 3, 8), (hb.K1_BF16, 100, 256, 0, 8), (hb.K1_BF16, 2**31, 256, 3, 8)):
        try:
            hb.k1_grid(*bad)
        except hb.MtqError:
            continue
        raise AssertionError(bad)


def test_every_group_can_claim_all_its_units():
    rng = np.random.default_rng(2024)
    seen = {}
    n = 0
    for kind in (hb.K1_BF16, hb.K1_DIRECT):
        W = WAVES_PER_BLOCK[kind]
        for cus in CUS:
            for wps in WAVES_PER_SIMD:
                for upw in QUOTAS:
                    totals = _borders(cus, wps, W, upw * QUOTA_SCALE[kind])
                    totals |= {64 * k + d for k in (1, 2, 100, 8191) for d in (-1, 1)} | {524288}
                    totals |= {int(v) for v in rng.integers(1, 1 << int(rng.integers(2, 31)), size=6)}
                    for total in sorted(totals):
                        regime = _check(kind, total, cus, wps, upw)
                        seen[(kind, regime)] = seen.get((kind, regime), 0) + 1
                        n += 1
    for kind in (hb.K1_BF16, hb.K1_DIRECT):
        for regime in ("resident", "quota", "oversubscribed", "persistent"):
            assert seen.get((kind, regime), 0) > 100, (kind, regime, seen)
    assert n > 20000


def test_this_process_uses_the_documented_defaults():
    """Negative switches stand for the process's own: 8 units per wave, 3 waves per SIMD for both kernels - unless the environment says
    otherwise (the library reads its switches once, so this only holds where they are unset)."""
    import os

    if any(k in os.environ for k in ("MTQ_K1_UNITS_PER_WAVE", "MTQ_K1_WAVES")):
        return
    for kind in (hb.K1_BF16, hb.K1_DIRECT):
        for total in (1, 1000, 22528, 22529, 400000, 2097152):
            assert hb.k1_grid(kind, total, 256) == hb.k1_grid(kind, total, 256, 3, 8)
