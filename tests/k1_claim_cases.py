"""K1 work-claim cases shared by tests/test_k1_work_claim_gpu.py and its child processes (not collected by pytest):
    python tests/k1_claim_cases.py            one JSON line: every launch with its regime, the mismatches, the ring's state
K1 hands its units out through device counters (csrc/mtq_fast.hip, csrc/mtq_direct.hip); a mistake there is a unit NOBODY computes,
and a record buffer that is reused then still shows the previous, correct answer.  So every launch here writes into a buffer filled
with one NaN pattern no kernel writes (SENTINEL), and is then checked twice: no promised double still holds the pattern ("unit not
computed", an integer compare, reported with the unit), and every record has the oracle's bits.  Inputs are finite; the tiles the
exact routes cannot take (groups scaled by 1e-28, a 2e18 element) sit in the first, a middle and the last tensor and unit, so the
strided fix-up kernels run at every size too.

Sizes beyond what the oracle does in reasonable time are built from a few distinct blocks repeated (whole tensors in a shuffled
order, or one strip repeated along its row): `idx` maps every tile of the launch to the distinct record it must equal.

listed_cases() holds lists of at most 288 tiles, sorted, where every wave of a listed kernel takes one item; lists of more than two
rounds of each listed kernel (unsorted ones too, a claimed length above the capacity, hundreds of handed-back tiles) are in
tests/test_k1_listed_long_gpu.py, which builds its inputs with uniform_case.  K1T (the ring walk's fifth launch) on batches, views and
long redo lists is in tests/test_k1t_views_gpu.py."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
import torch  # noqa: E402

from oracle import mtq_oracle as orc  # noqa: E402
from quantization_analysis_amd import hip_backend as hb  # noqa: E402

ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
SENTINEL = 0x7FF8A5C35A3CA5C3      # not kRedoMagic, not the hole poison, not 0x7FBADBAD (tests/test_tall_tensors_gpu.py) twice over
POISON = 0x7FF8000000000BAD        # what a partial launch leaves in the slots it does not write (csrc/mtq_fast.hip)
REDO_MAGIC = 0x7FF8C0DE5EED0001
assert len({SENTINEL, POISON, REDO_MAGIC, 0x7FBADBAD7FBADBAD}) == 4
BF16, DIRECT = hb.K1_BF16, hb.K1_DIRECT
DEV = "cuda"                       # (a dry run of the case builders on the host sets "cpu")
KIND_NAME = {BF16: "bf16", DIRECT: "direct"}
PARTIAL = (0xE, 0x2, 0x4)          # layout, full, sums: what the streamed driver's lazy route asks of K1
STRIP_PERIOD = 127                 # units of the repeated strip: odd, so repeats never line up with the 64 counter groups
BLOCK_CAP = 64                     # units per distinct tensor of a repeated batch (the oracle does ~5 000 tiles per second)


def promised_columns(layout, full, sums=0, err=0):
    """tests/test_hip_kernels.py _promised_columns: the record columns a partial / listed launch promises (Σx, Σx² not included)."""
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


def sentinel_filled(shape):
    return torch.full(tuple(shape), SENTINEL, dtype=torch.int64, device=DEV).view(torch.float64)


def oracle_bits(x2d) -> torch.Tensor:
    """The oracle's full records (all four formats) of a 2-D device tensor, as int64 bits on the device."""
    rec = orc.tile_stats(np.ascontiguousarray(x2d.float().cpu().numpy()), ALL)
    return torch.from_numpy(rec.view(np.int64)).to(DEV)


def layout_columns(mask: int) -> list:
    """Columns of the full record that make up the record of layout `mask` (slots are independent of one another)."""
    return [0, 1] + [2 + 5 * f + k for f in range(4) if mask >> f & 1 for k in range(5)]


def prime_factors(n: int) -> list:
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1 if p == 2 else 2
    return out + ([n] if n > 1 else [])


def factor3(total: int, cap: int = BLOCK_CAP):
    """total = count * a * b with all three above 1 and a * b small (the distinct tensors go through the oracle), or None."""
    ps = prime_factors(total)
    if len(ps) < 3:
        return None
    a, b, rest = ps[0], ps[1], ps[2:]
    while len(rest) > 1 and a * b * rest[0] <= cap:
        if a <= b:
            a *= rest.pop(0)
        else:
            b *= rest.pop(0)
    if a * b > 32 * cap:
        return None
    return total // (a * b), a, b


class Case:
    """One input with the records every launch over it must produce.  x: (count, rows, cols) device tensor, or mats: the matrices of a
    ragged batch; idx[t]: row of `full` (the distinct tensors' oracle records, int64 bits) that tile t of the launch must equal;
    bad[t]: tile t goes through the literal fix-up; unit_of: tile -> work unit as the kernel numbers them."""

    def __init__(self, kind, total, what, idx, full, bad, unit_of, x=None, mats=None):
        self.kind, self.total, self.what, self.idx, self.full, self.bad, self.unit_of, self.x, self.mats = kind, total, what, idx, full, bad, unit_of, x, mats
        assert int(idx.numel()) == int(bad.numel())

    def check(self, got, mask: int, route: str, cols=None, holes: bool = False) -> list:
        """→ failure descriptions (empty: every promised double was written and has the oracle's bits; holes hold the poison)."""
        rec = got.shape[-1]
        g = got.reshape(-1, rec).view(torch.int64)
        if g.shape[0] != self.idx.numel() or rec != hb.record_doubles(mask):
            return [f"{self.what} {route}: {tuple(got.shape)} records for {self.idx.numel()} tiles"]
        want_all = self.full[:, layout_columns(mask)]
        cols = list(range(rec)) if cols is None else sorted(set([0, 1] + list(cols)))
        colt = torch.tensor(cols, device=DEV)
        holet = torch.tensor([c for c in range(rec) if c not in cols], dtype=torch.int64, device=DEV)
        fails, step = [], 1 << 19
        missing_tiles, wrong_tiles, hole_tiles = [], [], []
        for s in range(0, g.shape[0], step):
            gi, wi = g[s:s + step], want_all[self.idx[s:s + step]]
            missing = (gi[:, colt] == SENTINEL).any(1)
            wrong = (gi[:, colt] != wi[:, colt]).any(1) & ~missing
            if bool(missing.any()):
                missing_tiles += (torch.nonzero(missing)[:, 0] + s).tolist()
            if bool(wrong.any()):
                wrong_tiles += (torch.nonzero(wrong)[:, 0] + s).tolist()
            if holes and holet.numel():
                hv = gi[:, holet]
                ok = (hv == POISON) | (self.bad[s:s + step, None] & (hv == wi[:, holet]))   # the literal fix-up writes the whole record
                if not bool(ok.all()):
                    hole_tiles += (torch.nonzero(~ok.all(1))[:, 0] + s).tolist()
        if missing_tiles:
            units = sorted({self.unit_of(t) for t in missing_tiles})
            fails.append(f"{self.what} {route}: unit not computed: {len(units)} units {units[:8]} ({len(missing_tiles)} tiles {missing_tiles[:8]})")
        if wrong_tiles:
            fails.append(f"{self.what} {route}: records differ from the oracle in {len(wrong_tiles)} tiles {wrong_tiles[:8]}")
        if hole_tiles:
            fails.append(f"{self.what} {route}: unwritten slots do not hold the poison in {len(hole_tiles)} tiles {hole_tiles[:8]}")
        return fails


def _rand(seed: int, shape, bf16: bool):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(tuple(shape), generator=g, device=DEV) * 0.02
    return x.to(torch.bfloat16) if bf16 else x


def _spoil(x, tile_row: int, col0: int, width: int, how: int) -> None:
    """Makes the tiles at (tile_row, col0 .. col0 + width) ones the exact routes hand to the literal route: groups below the exponent
    window (how 0) or one element above it (how 1).  Finite either way."""
    if how == 0:
        x[tile_row * 32:tile_row * 32 + 32, col0:col0 + width] *= 1e-28
    else:
        x[tile_row * 32 + 3, col0 + 5] = 2.0e18


def uniform_case(kind: int, total: int, seed: int, force=None, trim=(5, 9)) -> Case:
    """A uniform batch of `total` work items of that kernel: bf16 storage in 32x128 units (count, 32a, 128b) for the LDS-staged kernel,
    float32 storage with ragged edges in 32x32 tiles for the direct kernel.  count, a, b all above 1 where total factors that way
    (locate()'s three divisions), else one tensor of a single tile row.  force: (count, a, b, distinct) names the shape; trim: rows
    and columns the float32 tensors fall short of whole tiles."""
    if force:
        assert force[0] * force[1] * force[2] == total
    bf16 = kind == BF16
    uw, upt_tiles = (128, 4) if bf16 else (32, 1)                      # columns and tiles of a unit
    fac = force[:3] if force else factor3(total)
    if fac is not None:
        count, a, b = fac
        nd = force[3] if force else min(3, count)
        trim_r, trim_c = (0, 0) if bf16 else trim                      # float32 storage: ragged edges, unless the caller names the shape
        rows, cols = a * 32 - trim_r, b * uw - trim_c
        tiles_w = b * upt_tiles
        tiles = a * tiles_w
        bad_d = torch.zeros((nd, tiles), dtype=torch.bool, device=DEV)
        dist = [_rand(seed * 16 + d, (rows, cols), bf16) for d in range(nd)]
        sites = [(0, 0, 0, 0), (1 % nd, a // 2, b // 2, 1), (nd - 1, a - 1, b - 1, 0)]   # (distinct tensor, tile row, unit column, how)
        for d, tr, uc, how in sites:
            _spoil(dist[d], tr, uc * uw, uw, how)
            first = tr * tiles_w + uc * upt_tiles
            bad_d[d, first:first + (upt_tiles if how == 0 else 1)] = True
        full = torch.cat([oracle_bits(t) for t in dist])
        order = torch.from_numpy(np.random.default_rng(seed).integers(0, nd, size=count)).to(DEV)
        order[0], order[count // 2], order[count - 1] = 0, 1 % nd, nd - 1   # the spoiled units in the first, a middle and the last tensor
        x = torch.stack(dist)[order].contiguous()
        idx = (order[:, None] * tiles + torch.arange(tiles, device=DEV)[None, :]).reshape(-1)
        bad = bad_d[order].reshape(-1)
        shape = (count, rows, cols)

        def unit_of(t, _tiles=tiles, _tw=tiles_w, _a=a, _b=b):
            bi, r = divmod(t, _tiles)
            tr, tc = divmod(r, _tw)
            return bi * _a * _b + tr * _b + tc // upt_tiles
    else:
        p = min(total, STRIP_PERIOD)
        rows = 32 if bf16 else 27
        base = _rand(seed * 16, (rows, p * uw), bf16)
        last = (total - 1) % p
        bad_b = torch.zeros((p * upt_tiles,), dtype=torch.bool, device=DEV)
        for uc, how in ((0, 0), (p // 2, 1), (last, 0)):
            _spoil(base, 0, uc * uw, uw, how)
            bad_b[uc * upt_tiles:uc * upt_tiles + (upt_tiles if how == 0 else 1)] = True
        full = oracle_bits(base)
        x = base.repeat(1, -(-total // p))[:, :total * uw].contiguous()[None]
        idx = torch.arange(total * upt_tiles, device=DEV) % (p * upt_tiles)
        bad = bad_b[idx]
        shape = tuple(x.shape)

        def unit_of(t):
            return t // upt_tiles
    return Case(kind, total, f"{KIND_NAME[kind]} {total} units as {shape}", idx, full, bad, unit_of, x=x)


def ragged_case(total: int, seed: int, bf16: bool = False) -> Case:
    """A ragged batch (mtq_tile_stats_ragged, the direct kernel) of `total` tiles: up to 24 matrices of one tile row, all views of one
    strip of STRIP_PERIOD distinct tiles repeated; the last matrix takes the remainder."""
    n = min(hb.RAGGED_MAX, total)
    each, extra = divmod(total, n)
    longest = each + extra
    p = min(longest, STRIP_PERIOD)
    base = _rand(seed * 16 + 7, (27, p * 32), bf16)
    _spoil(base, 0, 0, 32, 0)
    _spoil(base, 0, (p // 2) * 32, 32, 1)
    bad_b = torch.zeros((p,), dtype=torch.bool, device=DEV)
    bad_b[0] = bad_b[p // 2] = True
    full = oracle_bits(base)
    strip = base.repeat(1, -(-longest // p))[:, :longest * 32].contiguous()
    mats = [strip[:, :each * 32] for _ in range(n - 1)] + [strip]
    idx = torch.cat([torch.arange(m.shape[1] // 32, device=DEV) % p for m in mats])
    return Case(DIRECT, total, f"ragged {'bf16' if bf16 else 'f32'} {total} tiles in {n} matrices", idx, full, bad_b[idx], lambda t: t, mats=mats)


# --------------------------------------------------------------------------------------------------------------- launches
def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def regime(kind: int, total: int) -> dict:
    blocks, quota, groups = hb.k1_grid(kind, total, cus())
    return {"kind": KIND_NAME[kind], "total": int(total), "regime": hb.k1_regime(kind, total, cus()), "blocks": blocks, "quota": quota, "groups": groups}


def launch(case: Case, route: str):
    """One launch of `case` on the current stream into sentinel-filled records → the arguments of case.check for it."""
    if route in ("batched_f", "batched_e"):
        mask = 0xF if route == "batched_f" else 0xE
        count, rows, cols = case.x.shape
        th, tw = hb.tiles_hw(rows, cols)
        out = sentinel_filled((count, th * tw, hb.record_doubles(mask)))
        hb.tile_stats_batched(case.x, mask, out=out)
        return out, mask, route, None, False
    if route in ("partial", "begin_end"):
        layout, full, sums = PARTIAL
        count, rows, cols = case.x.shape
        out = sentinel_filled((count, (rows // 32) * (cols // 32), hb.record_doubles(layout)))
        if route == "partial":
            hb.tile_stats_partial(case.x, layout, full, sums, out=out)
        else:
            mark = torch.zeros((1,), dtype=torch.int32, device=DEV)
            lid = hb.tile_stats_partial_begin(case.x, layout, full, sums, out, mark)
            hb.tile_stats_partial_end(case.x, layout, out, mark, lid)
        return out, layout, route, promised_columns(layout, full, sums), True
    if route == "ragged":
        out = sentinel_filled((case.total, hb.record_doubles(0xF)))
        hb.tile_stats_ragged(case.mats, 0xF, out=out)
        return out, 0xF, route, None, False
    raise ValueError(route)


def run_case(case: Case, routes, log: list) -> list:
    """Launches `case` through the named routes → failures; every launch is appended to `log` with the regime mtq_debug_k1_grid
    reports for it."""
    fails = []
    for route in routes:
        mine = case.check(*launch(case, route))
        log.append(dict(regime(case.kind, case.total), route=route, ok=not mine))
        fails += mine
    return fails


def border_totals(kind: int) -> list:
    """The regime borders of this process's geometry on this device, found through mtq_debug_k1_grid: the largest total with a wave per
    unit (R) and R + 1; the largest total whose grid is still the resident one (Q, where waves retire) and Q + 1; one below and one
    above a multiple of 64 x W x quota beyond those."""
    n_cu = cus()
    W = hb.k1_waves_per_block(kind)

    def largest(pred, lo=1, hi=(1 << 31) - 1):     # pred is true up to some total and false beyond it
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if pred(mid) else (lo, mid - 1)
        return lo

    R = largest(lambda t: hb.k1_regime(kind, t, n_cu) == "resident", hi=1 << 28)
    resident_blocks = hb.k1_grid(kind, R, n_cu)[0]
    quota = hb.k1_grid(kind, 1 << 28, n_cu)[1]
    # (without a quota the grid never grows beyond the resident one: no such border)
    Q = largest(lambda t: hb.k1_grid(kind, t, n_cu)[0] <= resident_blocks, hi=1 << 28) if quota else R
    m = 64 * W * max(quota, 1)
    k = (Q + 1) // m + 2
    return sorted({R, R + 1, Q, Q + 1, k * m - 1, k * m + 1})


def border_cases(log: list, ragged: bool = True) -> list:
    fails = []
    for kind, routes in ((BF16, ("batched_f", "begin_end")), (DIRECT, ("batched_f",))):
        for j, total in enumerate(border_totals(kind)):
            fails += run_case(uniform_case(kind, total, 100 + 10 * kind + j), routes, log)
            if kind == DIRECT and ragged:
                fails += run_case(ragged_case(total, 200 + j, bf16=j == 3), ("ragged",), log)
            torch.cuda.synchronize()
    return fails


def listed_cases() -> tuple:
    """The listed-completion cases of tests/test_hip_kernels.py test_partial_records_and_listed_completion against the ORACLE, for lists
    of 0, 1, 4k+1 and all tiles: the partial launch into sentinel-filled records, then mtq_tile_stats_listed through the exact-integer
    form (scratch given) and the one-wave-per-tile form → (failures, launches)."""
    rng = np.random.default_rng(5)
    count, rows, cols = 3, 256, 384
    T = (rows // 32) * (cols // 32)
    xs = [_rand(900 + i, (rows, cols), True) for i in range(count)]
    xs[0][:32, :128] = 0.0                                 # an all-zero unit
    xs[0][40, 130] = 3.0e4                                 # tail-class neighbours
    _spoil(xs[1], 0, 0, 32, 1)                             # the exact routes hand these tiles over
    _spoil(xs[2], 2, 256, 32, 0)
    xd = torch.stack(xs).contiguous()
    full = torch.cat([oracle_bits(t) for t in xs])
    fails, launches = [], 0
    for layout, fullm, sums, lfull, lerr in ((0xE, 0x2, 0x4, 0x8, 0x4), (0x6, 0x0, 0x2, 0x4, 0x2), (0xE, 0x6, 0x0, 0x8, 0x0), (0xC, 0x0, 0x4, 0x8, 0x4)):
        want = full[:, layout_columns(layout)]
        got = sentinel_filled((count, T, hb.record_doubles(layout)))
        hb.tile_stats_partial(xd, layout, fullm, sums, out=got)
        gflat = got.view(count * T, -1).view(torch.int64)
        cols_p = [0, 1] + promised_columns(layout, fullm, sums)
        if bool((gflat[:, cols_p] == SENTINEL).any()) or not torch.equal(gflat[:, cols_p], want[:, cols_p]):
            fails.append(f"listed: partial launch {layout:#x}/{fullm:#x}/{sums:#x} differs from the oracle")
        lcols = promised_columns(layout, lfull, err=lerr)
        other = [c for c in range(want.shape[1]) if c not in lcols]
        for n in (0, 1, 37, count * T):
            special = [T + 0, 2 * T + 2 * 12 + 8] if n == 37 else []                      # the handed-over tiles among the 4k+1
            pool = np.setdiff1d(np.arange(count * T), special)
            ids = np.sort(np.concatenate([rng.choice(pool, size=n - len(special), replace=False), special])).astype(np.int32)
            listed = torch.zeros((count * T,), dtype=torch.int32, device=DEV)
            listed[:ids.size] = torch.from_numpy(ids).to(DEV)
            nl = torch.tensor([ids.size], dtype=torch.int32, device=DEV)
            sel = torch.from_numpy(ids.astype(np.int64)).to(DEV)
            rest = torch.ones(count * T, dtype=torch.bool, device=DEV)
            rest[sel] = False
            for scratch in (torch.empty((count * T + 1,), dtype=torch.int32, device=DEV), None):
                work = got.clone()
                hb.tile_stats_listed(xd, layout, lfull, lerr, listed, nl, work, scratch=scratch)
                launches += 1
                w = work.view(count * T, -1).view(torch.int64)
                ok = torch.equal(w[sel][:, lcols], want[sel][:, lcols])                     # the listed tiles' statistics: the oracle's
                ok &= torch.equal(w[rest], gflat[rest]) and torch.equal(w[sel][:, other], gflat[sel][:, other])   # nothing else touched
                if not ok:
                    fails.append(f"listed: layout {layout:#x} full {lfull:#x} err {lerr:#x}, {ids.size} tiles, scratch {scratch is not None}")
    return fails, launches


def main() -> int:
    t0 = time.time()
    torch.cuda.set_device(0)
    hb.require_gpu()
    log = []
    fails = border_cases(log)
    lfails, listed_launches = listed_cases()
    fails += lfails
    torch.cuda.synchronize()
    print(json.dumps({"cus": cus(), "failures": fails, "launches": log, "listed_launches": listed_launches,
                      "counters_nonzero": hb.work_counters_nonzero(), "seconds": round(time.time() - t0, 1)}))
    return 1 if fails else 0


if __name__ == "__main__":
    raise SystemExit(main())
