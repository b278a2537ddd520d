"""Synthesized stats records that drive the greedy search's visit rounds down a chosen accept / reject course, and a plain sequential
reference of the search.  Imports no project code.

Record layout (include/mtq.h): columns 0, 1 are Σx, Σx²; then per format of the mask in code order (bf16 0, bfp8 1, bfp4 2, bfp2 3) the
five sums Σy, Σy², Σxy, Σ|x−y|, max|x−y|.  With MASK_IDENTITY (and bit 0 clear) the bf16 candidate is implied as (Σx, Σx², Σx², 0, 0).

The budget design: n = 2^20 and every running sum is an integer below 2^53, so no decision of the plain scan depends on rounding.
  mae: base Σ|x−y| = 2^20 per tile, B = T·2^20, thr = B / n (the base pass sits on the threshold); an accepted visit lands the running
       sum on B, B−1 or B−2, a rejected one on B+1.
  pcc: Σx = Σy = 0, Σx² = Σy² = 2^20 in every format, so the denominator is exactly 2^20; B = 3·2^18, thr = B / 2^20; the base Σxy
       totals B; an accepted visit lands Σxy on B, B+1 or B+2, a rejected one on B−1.
Every rejection misses by one unit and a third of the acceptances sit on the threshold: a running sum that is off by one flips a decision.
"""
from __future__ import annotations

import math

import numpy as np

N = float(1 << 20)
MASK_IDENTITY = 0x10
Y, Y2, XY, AB, MX = range(5)
JUNK = float(1 << 30)      # in every column no search may read


def rec_len(mask: int) -> int:
    return 2 + 5 * bin(mask & 0xF).count("1")


def col(mask: int, f: int, which: int):
    """Record column of sum `which` of format f; for the implied bf16 the x column that stands in for it, None for its zeros."""
    if f == 0 and (mask & MASK_IDENTITY) and not (mask & 1):
        return (0, 1, 1, None, None)[which]
    assert (mask >> f) & 1, (mask, f)
    return 2 + 5 * bin(mask & ((1 << f) - 1)).count("1") + which


def column(rec: np.ndarray, mask: int, f: int, which: int) -> list:
    c = col(mask, f, which)
    return [0.0] * rec.shape[0] if c is None else rec[:, c].tolist()


# ----------------------------------------------------------------------------------------------------------------------------------
# The plain reference: the sequential algorithm in Python floats
# ----------------------------------------------------------------------------------------------------------------------------------
def plain_scan(rec: np.ndarray, mask: int, formats, metric: str, thr: float, n: float, seed: int, zero_rule: str = "status") -> dict:
    """→ {"status", "map", "fixed_before"}: fixed_before[p] is the `fixed` vector as pass p found it (the search's candidates then).
    zero_rule "status": a zero denominator at an evaluated visit ends the search with status 1 and no map (the device's contract);
    "sumabs": the value is 1 if Σ|x−y| == 0 else 0 (the host scan's rule)."""
    if metric == "atol":
        return plain_atol(rec, mask, formats, thr, seed)
    T = rec.shape[0]
    mae = metric == "mae"
    x, x2 = rec[:, 0].tolist(), rec[:, 1].tolist()
    ab = {f: column(rec, mask, f, AB) for f in formats}
    y = {f: column(rec, mask, f, Y) for f in formats}
    y2 = {f: column(rec, mask, f, Y2) for f in formats}
    xy = {f: column(rec, mask, f, XY) for f in formats}
    base = formats[0]
    sx = sx2 = sy = sy2 = sxy = sab = 0.0
    for t in range(T):                       # initial sums, in tile order
        sx += x[t]; sx2 += x2[t]; sy += y[base][t]; sy2 += y2[base][t]; sxy += xy[base][t]; sab += ab[base][t]

    class Zero(Exception):
        pass

    def good(cy, cy2, cxy, cab):
        if mae:
            return cab / n <= thr
        mean_x = sx / n
        mean_y = cy / n
        am2 = sx2 - n * mean_x * mean_x
        bm2 = cy2 - n * mean_y * mean_y
        am2 = 0.0 if am2 < 0.0 else am2
        bm2 = 0.0 if bm2 < 0.0 else bm2
        denom = math.sqrt(am2 * bm2)
        if denom == 0.0:
            if zero_rule == "status":
                raise Zero
            return (1.0 if cab == 0.0 else 0.0) >= thr
        return (cxy - n * mean_x * mean_y) / denom >= thr

    rng = np.random.default_rng(seed)
    assign = [base] * T
    fixed = np.zeros(T, dtype=bool)
    fixed_before = []
    try:
        for p, f in enumerate(formats):
            fixed_before.append(fixed.copy())
            cand = np.where(~fixed)[0]
            if cand.size == 0:
                break
            order = rng.permutation(cand)
            if p == 0:                       # every tile has the base format: one question for all of them
                if not good(sy, sy2, sxy, sab):
                    fixed[:] = True
                continue
            for t in order.tolist():
                c = assign[t]
                ny, ny2, nxy, nab = sy + (y[f][t] - y[c][t]), sy2 + (y2[f][t] - y2[c][t]), sxy + (xy[f][t] - xy[c][t]), sab + (ab[f][t] - ab[c][t])
                if good(ny, ny2, nxy, nab):
                    sy, sy2, sxy, sab = ny, ny2, nxy, nab
                    assign[t] = f
                else:
                    fixed[t] = True
    except Zero:
        return {"status": 1, "map": None, "fixed_before": fixed_before}
    while len(fixed_before) < len(formats):
        fixed_before.append(fixed.copy())
    return {"status": 0, "map": np.array(assign, dtype=np.int8), "fixed_before": fixed_before}


def plain_atol(rec: np.ndarray, mask: int, formats, thr: float, seed: int) -> dict:
    """The atol search, literally: a visit is accepted iff the candidate's maximum and every OTHER tile's current maximum are <= thr,
    the maximum over the others recomputed at every visit.  A NaN maximum in a listed format: status 1 (the device's contract)."""
    T = rec.shape[0]
    mx = {f: np.array(column(rec, mask, f, MX), dtype=np.float64) for f in formats}
    if any(np.isnan(v).any() for v in mx.values()):
        return {"status": 1, "map": None, "fixed_before": []}
    base = formats[0]
    cur = mx[base].copy()
    assign = np.full(T, base, dtype=np.int8)
    fixed = np.zeros(T, dtype=bool)
    rng = np.random.default_rng(seed)
    for p, f in enumerate(formats):
        cand = np.where(~fixed)[0]
        if cand.size == 0:
            break
        order = rng.permutation(cand)
        if p == 0:
            if not float(np.max(cur)) <= thr:
                fixed[:] = True
            continue
        for t in order.tolist():
            others = np.delete(cur, t)
            if mx[f][t] <= thr and (others.size == 0 or float(np.max(others)) <= thr):
                cur[t] = mx[f][t]
                assign[t] = f
            else:
                fixed[t] = True
    return {"status": 0, "map": assign, "fixed_before": []}


# ----------------------------------------------------------------------------------------------------------------------------------
# Patterns: (pass, visit index, candidates of the pass, tile) → accept?
# ----------------------------------------------------------------------------------------------------------------------------------
def all_accept(p, k, nc, t):
    return True


def all_reject(p, k, nc, t):
    return False


def one_reject(r, at_pass=1):
    return lambda p, k, nc, t: not (p == at_pass and k == r)


def one_accept(a, at_pass=1):
    return lambda p, k, nc, t: k == a if p == at_pass else True


def periodic(word: str):
    return lambda p, k, nc, t: word[k % len(word)] == "A"


def bernoulli(q: float, seed: int):
    drawn = {}

    def pat(p, k, nc, t):
        if (p, nc) not in drawn:
            drawn[(p, nc)] = np.random.default_rng([seed, p]).random(nc) < q
        return bool(drawn[(p, nc)][k])
    return pat


def reject_tile(tile: int, at_pass=1):
    return lambda p, k, nc, t: not (p == at_pass and t == tile)


def per_pass(table: dict, default=all_accept):
    return lambda p, k, nc, t: table.get(p, default)(p, k, nc, t)


# ----------------------------------------------------------------------------------------------------------------------------------
# The builder
# ----------------------------------------------------------------------------------------------------------------------------------
def blank_records(T: int, mask: int, metric: str) -> np.ndarray:
    rec = np.full((T, rec_len(mask)), JUNK if metric == "mae" else -JUNK, dtype=np.float64)
    if metric == "pcc":
        rec[:, 0] = 0.0
        rec[:, 1] = 1.0
        rec[0, 1] = N - (T - 1)
        for f in range(4):
            if (mask >> f) & 1:
                rec[:, col(mask, f, Y)] = 0.0
                rec[:, col(mask, f, Y2)] = rec[:, 1]
                rec[:, col(mask, f, AB)] = 1.0
                rec[:, col(mask, f, MX)] = 1.0
    return rec


def build_budget_case(T: int, mask: int, formats, metric: str, seed: int, pattern, land_seed: int = 0, base_fail: bool = False, check: bool = True) -> dict:
    """Records whose search takes the course `pattern` asks for, visit by visit → the case: records, thr, n, the designed map, the trace
    [(pass, visit, tile, accepted)].  Asserts that the plain scan reproduces the designed map."""
    assert metric in ("mae", "pcc") and seed != 0
    formats = list(formats)
    mae = metric == "mae"
    which = AB if mae else XY
    sign = -1 if mae else 1                       # an accepted visit lands on B + sign·{0, 1, 2}, a rejected one on B − sign
    base = formats[0]
    rec = blank_records(T, mask, metric)
    identity_base = col(mask, base, MX) is None
    if mae:
        B = T * (1 << 20)
        S = 0
        if not identity_base:
            rec[:, col(mask, base, AB)] = float(1 << 20)
            S = B
        thr = (B - 1) / N if base_fail else B / N
    else:
        B = 3 << 18
        S = 1 << 20
        if not identity_base:
            S = B - 1 if base_fail else B
            q = S // T
            rec[:, col(mask, base, XY)] = float(q)
            rec[0, col(mask, base, XY)] = float(q + S - q * T)
        thr = B / N
    assert not (base_fail and identity_base), "the implied bf16 sums are what they are: its base pass cannot be made to fail by one unit"

    def value(t, f):
        c = col(mask, f, which)
        return 0.0 if c is None else float(rec[t, c])

    rng = np.random.default_rng(seed)
    land = np.random.default_rng([land_seed, T, seed])
    assign = np.full(T, base, dtype=np.int8)
    fixed = np.zeros(T, dtype=bool)
    trace = []
    for p, f in enumerate(formats):
        cand = np.where(~fixed)[0]
        if cand.size == 0:
            break
        order = rng.permutation(cand)
        if p == 0:
            if base_fail:
                fixed[:] = True
            continue
        fc = col(mask, f, which)
        assert fc is not None, "the implied bf16 can only be the base of a designed case"
        lands = land.integers(0, 3, size=order.size).tolist()
        for k, t in enumerate(order.tolist()):
            acc = bool(pattern(p, k, int(order.size), t))
            S2 = B + sign * lands[k] if acc else B - sign
            rec[t, fc] = value(t, int(assign[t])) + float(S2 - S)
            trace.append((p, k, t, acc))
            if acc:
                S = S2
                assign[t] = f
            else:
                fixed[t] = True
    assert float(np.abs(rec[np.isfinite(rec)]).max()) < 2.0 ** 53
    case = {"records": rec, "thr": thr, "n": N, "map": assign, "status": 0, "seed": seed, "mask": mask, "formats": formats, "metric": metric,
            "trace": trace, "T": T}
    if check:
        verify(case)
    return case


def verify(case: dict) -> dict:
    """The builder's own assertion: the plain scan takes the designed course."""
    got = plain_scan(case["records"], case["mask"], case["formats"], case["metric"], case["thr"], case["n"], case["seed"])
    assert got["status"] == case["status"], (case.get("name"), got["status"])
    if case["status"] == 0:
        assert np.array_equal(got["map"], case["map"]), (case.get("name"), int((got["map"] != case["map"]).sum()))
    case["fixed_before"] = got["fixed_before"]
    return case


def perturbed(case: dict, visit: int, by: float) -> np.ndarray:
    """The case's records with `by` added to the delta of trace entry `visit`."""
    p, _k, t, _acc = case["trace"][visit]
    rec = case["records"].copy()
    rec[t, col(case["mask"], case["formats"][p], AB if case["metric"] == "mae" else XY)] += by
    return rec


# ----------------------------------------------------------------------------------------------------------------------------------
# The speculative zero denominator (pcc, formats [0, 1], mask 0x3)
# ----------------------------------------------------------------------------------------------------------------------------------
def _pass1_order(T: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    rng.permutation(T)                             # the base pass's draw
    return rng.permutation(T).tolist()


def _zero_blank(T: int) -> np.ndarray:
    rec = np.zeros((T, rec_len(0x3)), dtype=np.float64)
    rec[:, 1] = 1.0
    rec[0, 1] = N - (T - 1)                        # Σx = 0, Σx² = 2^20
    rec[:, col(0x3, 0, AB)] = 1.0                  # Σ|x−y| never zero: the host's rule for a zero denominator then says "value 0"
    rec[:, col(0x3, 1, AB)] = 2.0
    return rec


def build_zero_accept_mode(T: int, j: int, seed: int, real: bool = False) -> dict:
    """Accept mode: visit j (tile tj) is rejected; lane j+1 (tile tn) holds visit j's delta in its speculative sums and has denominator
    zero there — its true sums do not.  Every tile takes the candidate except tj.  real: all y energy sits on tn and its candidate is
    zero, so the zero denominator is the true one: status 1."""
    order = _pass1_order(T, seed)
    tj, tn = order[j], order[j + 1]
    rec = _zero_blank(T)
    c_y2, c_xy = col(0x3, 0, Y2), col(0x3, 0, XY)
    if real:
        rec[tn, c_y2] = N
        rec[tn, c_xy] = 0.9 * N
    else:
        rec[tj, c_y2] = N - 4.0
        rec[tn, c_y2] = 4.0
        rec[tj, c_xy] = 0.9 * N
    want = np.ones(T, dtype=np.int8)
    want[tj] = 0
    case = {"records": rec, "thr": 0.75, "n": N, "map": None if real else want, "status": 1 if real else 0, "seed": seed, "mask": 0x3,
            "formats": [0, 1], "metric": "pcc", "T": T}
    return verify(case)


def build_zero_reject_mode(T: int, j: int, seed: int, real: bool = False) -> dict:
    """Reject mode (visit 0 is rejected): visits 1..j−1 are rejected, visit j is accepted and changes Σy²; lane j+1 (tile tn, which holds
    all of the base's y energy and whose candidate has none) has denominator zero against the OLD sums only.  real: no accept at j, so
    visit j+1 truly meets the zero denominator: status 1."""
    order = _pass1_order(T, seed)
    tj, tn = order[j], order[j + 1]
    assert j >= 1
    rec = _zero_blank(T)
    rec[tn, col(0x3, 0, Y2)] = N
    rec[tn, col(0x3, 0, XY)] = 0.9 * N
    rec[:, col(0x3, 1, XY)] = -0.5 * N             # (0.9 − 0.5) < 0.75: rejected
    rec[tn, col(0x3, 1, XY)] = 0.0
    if not real:
        rec[tj, col(0x3, 1, Y2)] = 12.0
        rec[tj, col(0x3, 1, XY)] = 0.0
    want = np.zeros(T, dtype=np.int8)
    want[tj] = 1
    case = {"records": rec, "thr": 0.75, "n": N, "map": None if real else want, "status": 1 if real else 0, "seed": seed, "mask": 0x3,
            "formats": [0, 1], "metric": "pcc", "T": T}
    return verify(case)


# ----------------------------------------------------------------------------------------------------------------------------------
# Half-ulp cases: the only ones that depend on the ORDER of the additions — and exact all the same
# ----------------------------------------------------------------------------------------------------------------------------------
BIG = 2.0 ** 60          # ulp 256 above, 128 below


def _sequential(v) -> float:
    s = 0.0
    for a in v.tolist():
        s += a
    return s


def build_half_ulp(T: int, metric: str, seed: int, identity: bool = False) -> dict:
    """mae: base Σ|x−y| is 2^60 on tile 0 and 128 elsewhere, the candidate's 2^60 and 256; thr = 2^60 / n.  Added one after the other,
    each +128 is a tie that rounds back to 2^60 and everything is accepted; any two addends grouped make 2^60 + 256, which rejects.
    pcc: the same on Σxy from above the threshold: −64 is the tie below 2^60 (−128 is representable there), base −64 and candidate
    −128 per tile.  pcc with the implied bf16 base (the two-chain initial sums): Σx² is 2^60 on tile 0 and 128 elsewhere, so the true
    Σx² = Σy² = Σxy = 2^60; tile 5's candidate takes Σxy to 3·2^58 − 256, one ulp below thr = 0.75, and is rejected — with initial
    sums of 2^60 + anything it would be accepted."""
    assert T > 64 and seed != 0
    if metric == "mae":
        mask, formats = 0x3, [0, 1]
        rec = blank_records(T, mask, "mae")
        b, c = col(mask, 0, AB), col(mask, 1, AB)
        rec[:, b] = 128.0
        rec[:, c] = 256.0
        rec[0, b] = rec[0, c] = BIG
        thr = BIG / N
        want = np.ones(T, dtype=np.int8)
        watched = rec[:, b]
    elif not identity:
        mask, formats = 0x3, [0, 1]
        rec = blank_records(T, mask, "pcc")
        b, c = col(mask, 0, XY), col(mask, 1, XY)
        rec[:, b] = -64.0
        rec[:, c] = -128.0
        rec[0, b] = rec[0, c] = BIG
        thr = BIG / N
        want = np.ones(T, dtype=np.int8)
        watched = rec[:, b]
    else:
        mask, formats = 0xE | MASK_IDENTITY, [0, 1]
        rec = blank_records(T, mask, "pcc")
        rec[:, 1] = 128.0
        rec[0, 1] = BIG
        rec[:, col(mask, 1, Y2)] = rec[:, 1]
        rec[:, col(mask, 1, XY)] = rec[:, 1]
        rec[5, col(mask, 1, XY)] = 128.0 - (2.0 ** 58 + 256.0)
        thr = 0.75
        want = np.ones(T, dtype=np.int8)
        want[5] = 0
        watched = rec[:, 1]
    assert _sequential(watched) == BIG and float(np.sum(watched)) != BIG, "the base column's sum must depend on the order of its additions"
    case = {"records": rec, "thr": thr, "n": N, "map": want, "status": 0, "seed": seed, "mask": mask, "formats": formats, "metric": metric, "T": T}
    return verify(case)


# ----------------------------------------------------------------------------------------------------------------------------------
# atol: synthesized maxima
# ----------------------------------------------------------------------------------------------------------------------------------
ATOL_THR = 0.125


def build_atol(T: int, mask: int, formats, seed: int, kind: str = "mixed") -> dict:
    """Maxima drawn from {thr/2, thr, the double above thr, 4·thr} for every format but the base, whose maxima stay within thr.
    kind "base_over": one tile's base maximum is one ulp above thr (every tile stays at the base); "nan_listed": a NaN in a listed
    format (status 1); "nan_unlisted": a NaN in a format of the mask that is not in the list (status 0)."""
    formats = list(formats)
    g = np.random.default_rng([seed, T])
    above = math.nextafter(ATOL_THR, math.inf)
    rec = np.full((T, rec_len(mask)), JUNK, dtype=np.float64)
    rec[:, 0] = 0.0
    for f in range(4):
        if (mask >> f) & 1:
            rec[:, col(mask, f, MX)] = np.array([ATOL_THR / 2, ATOL_THR, above, 4 * ATOL_THR])[g.integers(0, 4, size=T)]
    base = formats[0]
    bc = col(mask, base, MX)
    if bc is not None:
        rec[:, bc] = np.array([ATOL_THR / 2, ATOL_THR])[g.integers(0, 2, size=T)]
    where = int(g.integers(0, T))
    if kind == "base_over":
        assert bc is not None
        rec[where, bc] = above
    elif kind == "nan_listed":
        rec[where, col(mask, formats[-1], MX)] = math.nan
    elif kind == "nan_unlisted":
        spare = [f for f in range(4) if (mask >> f) & 1 and f not in formats]
        rec[where, col(mask, spare[0], MX)] = math.nan
    else:
        assert kind == "mixed"
    got = plain_atol(rec, mask, formats, ATOL_THR, seed)
    return {"records": rec, "thr": ATOL_THR, "n": N, "map": got["map"], "status": got["status"], "seed": seed, "mask": mask, "formats": formats,
            "metric": "atol", "T": T, "kind": kind}


# ----------------------------------------------------------------------------------------------------------------------------------
# The case list
# ----------------------------------------------------------------------------------------------------------------------------------
FULL = 0xF
IDENT = 0xE | MASK_IDENTITY


def budget_specs() -> list:
    """(name, T, mask, formats, metric, pattern, base_fail) of every designed course; the seed is the route's to choose."""
    out = []

    def add(name, T, mask, formats, pattern, metrics=("mae", "pcc"), base_fail=False):
        for m in metrics:
            out.append({"name": f"{name}-T{T}-{m}", "T": T, "mask": mask, "formats": list(formats), "metric": m, "pattern": pattern, "base_fail": base_fail})

    for T in (1, 15, 16, 17, 79, 80, 81, 143, 144, 145, 207, 208, 209, 272, 273):
        add("all_accept", T, FULL, [0, 1], all_accept)
    for r in (0, 1, 15, 16, 17, 79, 80, 143, 144, 207, 208, 271, 399):
        add(f"one_reject_{r}", 400, FULL, [0, 1], one_reject(r))
    for a in (0, 1, 63, 64, 65, 128, 129, 256, 257, 384, 699):
        add(f"one_accept_{a}", 700, FULL, [0, 1], one_accept(a))
    for T in (1, 2, 128, 129, 130, 256, 257, 258, 385):
        add("all_reject", T, FULL, [0, 1], all_reject)
    for T in (100, 513, 1000):
        for word in ("AR", "AARR", "AAR", "A" * 63 + "R", "A" * 64 + "R", "R" * 127 + "A", "R" * 128 + "A"):
            tag = word if len(word) < 8 else f"{len(word) - 1}{word[0]}+{word[-1]}"
            add(f"periodic_{tag}", T, FULL, [0, 1], periodic(word))
        for i, q in enumerate((1 / 16, 1 / 2, 15 / 16)):
            add(f"bernoulli_{i}", T, FULL, [0, 1], bernoulli(q, 40 + i))
    lists = (("full", FULL, [0, 1, 2, 3]), ("down", FULL, [2, 1, 0]), ("f13", FULL, [1, 3]), ("f30", FULL, [3, 0]), ("ident", IDENT, [0, 1, 2, 3]),
             ("ident03", IDENT, [0, 3]))
    for tag, mask, fl in lists:
        for T in (130, 577):
            if len(fl) > 2:   # pass 1 accepts everything, a pattern in pass 2 (with shared orders: the helper wave's second order)
                add(f"{tag}_p2_bernoulli", T, mask, fl, per_pass({2: bernoulli(0.5, 50)}))
                add(f"{tag}_p2_one_reject_64", T, mask, fl, per_pass({2: one_reject(64, 2)}))
                add(f"{tag}_p2_all_reject", T, mask, fl, per_pass({2: all_reject}))
            for tile in (0, 63, 64, T - 1):   # pass 2 then shuffles its own T−1 candidates
                add(f"{tag}_p1_reject_tile{tile}", T, mask, fl, reject_tile(tile))
            add(f"{tag}_p1_all_reject", T, mask, fl, per_pass({1: all_reject}))
            if mask == FULL:
                add(f"{tag}_base_fails", T, mask, fl, all_accept, base_fail=True)
        for T in (511, 512, 513, 577, 1025):  # the sift_map (512) and gather_deltas (256) edges on the own-candidates route
            add(f"{tag}_p1_bernoulli", T, mask, fl, per_pass({1: bernoulli(0.5, 60)}))
    for T in (64, 128, 256, 512, 640, 641):   # whole blocks of every loop: init_sums 4·64 / 10·64, gather 256, sift 512
        add("block_edges", T, FULL, [0, 1, 2], per_pass({1: bernoulli(0.75, 70), 2: bernoulli(0.5, 71)}))
        add("block_edges_ident", T, IDENT, [0, 1, 2], per_pass({1: bernoulli(0.75, 70), 2: bernoulli(0.5, 71)}))
    return out


def order_route_specs() -> list:
    """The two sides of the LDS / global-scratch order threshold."""
    return [{"name": f"order_route-T{T}-{m}", "T": T, "mask": 0x3, "formats": [0, 1], "metric": m, "pattern": bernoulli(0.5, 80), "base_fail": False}
            for T in (32768, 32769) for m in ("mae", "pcc")]


def build_spec(spec: dict, seed: int) -> dict:
    case = build_budget_case(spec["T"], spec["mask"], spec["formats"], spec["metric"], seed, spec["pattern"], base_fail=spec["base_fail"])
    case["name"] = f"{spec['name']}-seed{seed}"
    return case


ZERO_PLACES = ((32, 5), (200, 100), (200, 16 + 64 + 63))           # (T, j): a span-16 round, a run round, a run round's last lane
ZERO_REJECT_PLACES = ((32, 5), (300, 1 + 10), (300, 1 + 64 + 10), (300, 1 + 128 + 63))   # general round; rejecting run window a, window b, second step


def special_cases(seed: int) -> list:
    """Speculative and true zero denominators in both modes, and the half-ulp cases."""
    out = []
    for real in (False, True):
        for T, j in ZERO_PLACES:
            c = build_zero_accept_mode(T, j, seed, real)
            c["name"] = f"zero_accept_mode-T{T}-j{j}-{'real' if real else 'speculative'}-seed{seed}"
            out.append(c)
        for T, j in ZERO_REJECT_PLACES:
            c = build_zero_reject_mode(T, j, seed, real)
            c["name"] = f"zero_reject_mode-T{T}-j{j}-{'real' if real else 'speculative'}-seed{seed}"
            out.append(c)
    for T in (300, 641):
        for metric, ident in (("mae", False), ("pcc", False), ("pcc", True)):
            c = build_half_ulp(T, metric, seed, ident)
            c["name"] = f"half_ulp-T{T}-{metric}{'-ident' if ident else ''}-seed{seed}"
            out.append(c)
    return out


def atol_cases(seed: int) -> list:
    out = []
    lists = ((FULL, [0, 1, 2, 3]), (FULL, [1]), (FULL, [3, 1]), (FULL, [2, 0, 3]), (IDENT, [0, 1, 2, 3]), (IDENT, [0, 2]), (0x6, [1, 2]))
    for T in (1, 255, 256, 257, 1000):
        for mask, fl in lists:
            kinds = ["mixed"]
            if col(mask, fl[0], MX) is not None:
                kinds.append("base_over")
            if len(fl) > 1:
                kinds.append("nan_listed")
            if any((mask >> f) & 1 and f not in fl for f in range(4)):
                kinds.append("nan_unlisted")
            for kind in kinds:
                c = build_atol(T, mask, fl, seed, kind)
                c["name"] = f"atol-{kind}-T{T}-mask{mask:#x}-{''.join(map(str, fl))}-seed{seed}"
                out.append(c)
    return out


def group_key(case: dict):
    return (case["T"], case["mask"], tuple(case["formats"]), case["metric"], case["thr"], case["n"])


def grouped(cases) -> dict:
    """Cases with equal (T, mask, list, metric, thr, n): one launch of many tensors each."""
    groups = {}
    for c in cases:
        groups.setdefault(group_key(c), []).append(c)
    return groups


_CACHE = {}


def own_seed_cases() -> list:
    """Every designed course, special case and half-ulp case, each tensor with a seed of its own.  Built once per process."""
    if "own" not in _CACHE:
        cases = [build_spec(s, 1000 + 7 * i) for i, s in enumerate(budget_specs())]
        for seed in (11, 12):
            cases += special_cases(seed)
        _CACHE["own"] = cases
    return _CACHE["own"]


def shared_seed_cases(seed: int = 77, other: int = 78) -> list:
    """The same courses under ONE seed (a launch that shares its visiting orders), plus per (T, list, metric) group one tensor whose seed
    differs from the orders' seed: it must shuffle for itself."""
    key = ("shared", seed, other)
    if key not in _CACHE:
        specs = budget_specs()
        cases = [build_spec(s, seed) for s in specs] + special_cases(seed)
        seen = set()
        for s in specs:
            k = (s["T"], s["mask"], tuple(s["formats"]), s["metric"], s["base_fail"])
            if k not in seen and "bernoulli" in s["name"]:
                seen.add(k)
                cases.append(build_spec(s, other))
        _CACHE[key] = cases
    return _CACHE[key]


def order_route_cases(seed: int) -> list:
    key = ("route", seed)
    if key not in _CACHE:
        _CACHE[key] = [build_spec(s, seed) for s in order_route_specs()]
    return _CACHE[key]
