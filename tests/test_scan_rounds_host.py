"""CPU-only: the synthesized visit-round cases of tests/scan_round_cases.py through the host scan.  Every case has
already passed the builder's own assertion (the plain sequential scan takes the designed course); here the host library must take it
too, the host's rule for a zero denominator is checked against the plain scan under that rule, and the cases are shown to be
knife-edged: one unit on one accepted visit's delta changes the map."""
import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from tests import scan_round_cases as sc

NAMES = ["bf16", "bfp8", "bfp4", "bfp2"]


def names(case):
    return [NAMES[f] for f in case["formats"]]


def host_map(case, rec=None):
    amap, counts, _cols = hb.greedy_run(case["records"] if rec is None else rec, case["mask"], names(case), case["metric"], case["thr"], case["n"], case["seed"])
    return amap, np.array([counts[f] for f in NAMES])


def test_builder_covers_every_pattern_family():
    cases = sc.own_seed_cases()
    got = {c["name"].split("-")[0] for c in cases}
    for family in ("all_accept", "one_reject_0", "one_reject_399", "one_accept_0", "one_accept_699", "all_reject", "periodic_63A+R", "periodic_128R+A",
                   "bernoulli_1", "full_p2_bernoulli", "ident_p1_reject_tile63", "down_p1_all_reject", "f13_base_fails", "ident03_p1_bernoulli",
                   "block_edges", "zero_accept_mode", "zero_reject_mode", "half_ulp"):
        assert family in got, family
    assert {c["T"] for c in cases} >= {1, 15, 16, 17, 64, 79, 80, 81, 128, 143, 144, 145, 207, 208, 209, 256, 272, 273, 511, 512, 513, 577, 640, 641, 1025}
    assert len({c["seed"] for c in cases}) > 400


def test_host_scan_takes_the_designed_course():
    n = 0
    for c in sc.own_seed_cases() + sc.shared_seed_cases():
        if c["status"] != 0:
            continue
        amap, counts = host_map(c)
        assert np.array_equal(amap, c["map"]), (c["name"], int((amap != c["map"]).sum()))
        assert np.array_equal(counts, np.bincount(c["map"], minlength=4)), c["name"]
        n += 1
    assert n > 900


def test_host_scan_batched():
    """mtq_greedy_run_batch over every group of equal (T, mask, list, metric, thr, n)."""
    for key, cs in sc.grouped([c for c in sc.own_seed_cases() if c["status"] == 0]).items():
        maps, counts, _o = hb.greedy_run_batch(np.stack([c["records"] for c in cs]), cs[0]["mask"], names(cs[0]), cs[0]["metric"], cs[0]["thr"], cs[0]["n"],
                                               [c["seed"] for c in cs], 4)
        for i, c in enumerate(cs):
            assert np.array_equal(maps[i], c["map"]), c["name"]
            assert np.array_equal(counts[i], np.bincount(c["map"], minlength=4)), c["name"]


def test_host_zero_denominator_rule():
    """Where the plain scan says "zero denominator" (status 1 on the device) the host applies the reference's rule — the value is 1 if
    Σ|x−y| == 0 and 0 otherwise — and goes on: its map is the plain scan's under that rule."""
    n = 0
    for c in sc.special_cases(11) + sc.special_cases(77):
        if c["status"] != 1:
            continue
        want = sc.plain_scan(c["records"], c["mask"], c["formats"], c["metric"], c["thr"], c["n"], c["seed"], zero_rule="sumabs")
        assert want["status"] == 0
        amap, _counts = host_map(c)
        assert np.array_equal(amap, want["map"]), c["name"]
        n += 1
    assert n == 2 * (len(sc.ZERO_PLACES) + len(sc.ZERO_REJECT_PLACES))


@pytest.mark.parametrize("metric", ["mae", "pcc"])
def test_cases_are_knife_edged(metric):
    """One unit more or less on the delta of the first accepted visit changes the plain scan's map (and the host's the same way)."""
    n = 0
    for c in sc.own_seed_cases():
        if c["metric"] != metric or c["formats"] != [0, 1] or not c["name"].startswith(("bernoulli_1", "periodic_AR", "periodic_AARR", "periodic_AAR")):
            continue
        first = next(i for i, v in enumerate(c["trace"]) if v[3])
        for by in (1.0, -1.0):
            rec = sc.perturbed(c, first, by)
            got = sc.plain_scan(rec, c["mask"], c["formats"], c["metric"], c["thr"], c["n"], c["seed"])
            assert got["status"] == 0 and not np.array_equal(got["map"], c["map"]), (c["name"], by)
            amap, _counts = host_map(c, rec)
            assert np.array_equal(amap, got["map"]), (c["name"], by)
        n += 1
    assert n == 12


def test_order_route_cases_host():
    for c in sc.order_route_cases(5):
        amap, _counts = host_map(c)
        assert np.array_equal(amap, c["map"]), c["name"]


def test_atol_cases_host():
    """The literal atol scan against the host's (which keeps the maximum with a multiplicity), NaN cases aside: those are the device's
    status to report."""
    n = 0
    for c in sc.atol_cases(5):
        if c["kind"].startswith("nan"):
            continue
        amap, counts = host_map(c)
        assert np.array_equal(amap, c["map"]), c["name"]
        assert np.array_equal(counts, np.bincount(c["map"], minlength=4)), c["name"]
        if c["kind"] == "base_over":
            assert (c["map"] == c["formats"][0]).all(), c["name"]
        n += 1
    assert n >= 60
