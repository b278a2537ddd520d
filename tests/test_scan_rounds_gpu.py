"""The device greedy search (csrc/mtq_scan.hip) driven round by round from the synthesized records of tests/scan_round_cases.py
(DESIGN.md A.6zd): every case through every route that takes it — own shuffles, the launch's shared orders with the helper wave, the
search split in phases with the list of the last pass's candidates checked in between, and the atol walk.  The expected maps are the
designed ones, which a plain sequential scan that shares nothing with the code under test has reproduced; status, counts and maps are
compared exactly.  Cases with equal (T, mask, list, metric, thr, n) go into one launch of many tensors."""
import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from tests import scan_round_cases as sc

pytestmark = pytest.mark.gpu
NAMES = ["bf16", "bfp8", "bfp4", "bfp2"]


class Launch:
    """One group's tensors on the device with the buffers a search writes."""

    def __init__(self, cs):
        import torch

        self.cs = cs
        c = cs[0]
        self.T, self.count = c["T"], len(cs)
        self.args = (c["mask"], [NAMES[f] for f in c["formats"]], c["metric"], c["thr"], c["n"])
        self.recs = torch.from_numpy(np.stack([x["records"] for x in cs])).cuda()
        self.seeds = torch.tensor([x["seed"] for x in cs], dtype=torch.int64, device="cuda")
        self.maps = torch.full((self.count, self.T), -1, dtype=torch.int8, device="cuda")
        self.status = torch.full((self.count,), -1, dtype=torch.int32, device="cuda")
        self.counts = torch.full((self.count, 4), -1, dtype=torch.int32, device="cuda")
        self.scratch = torch.empty((hb.greedy_scan_scratch_bytes(self.count, self.T),), dtype=torch.uint8, device="cuda")

    def run(self, **kw):
        mask, formats, metric, thr, n = self.args
        hb.greedy_scan_device_ex(self.recs, mask, formats, metric, thr, n, self.seeds, self.maps, self.status, self.scratch, counts_out=self.counts, **kw)

    def check(self, route):
        import torch

        torch.cuda.synchronize()
        status, maps, counts = self.status.cpu().numpy(), self.maps.cpu().numpy(), self.counts.cpu().numpy()
        for i, c in enumerate(self.cs):
            assert status[i] == c["status"], (route, c["name"], int(status[i]))
            if c["status"] == 0:
                assert np.array_equal(maps[i], c["map"]), (route, c["name"], int((maps[i] != c["map"]).sum()), np.flatnonzero(maps[i] != c["map"])[:8].tolist())
                assert np.array_equal(counts[i], np.bincount(c["map"], minlength=4)), (route, c["name"])


def of_metric(cases, metric):
    return sc.grouped([c for c in cases if c["metric"] == metric])


@pytest.mark.parametrize("metric", ["mae", "pcc"])
def test_own_shuffles(metric):
    """mtq_greedy_scan_device: one wave per tensor, the order in LDS, a seed per tensor."""
    import torch

    for cs in of_metric(sc.own_seed_cases(), metric).values():
        L = Launch(cs)
        mask, formats, m, thr, n = L.args
        maps, status = hb.greedy_scan_device(L.recs, mask, formats, m, thr, n, L.seeds, counts_out=L.counts)
        L.maps, L.status = maps, status
        L.check("own shuffles")
    torch.cuda.synchronize()


@pytest.mark.parametrize("metric", ["mae", "pcc"])
def test_shared_orders(metric):
    """The launch's shared orders: two waves per tensor and the order of a tensor that shuffles for itself in global scratch, at any T.
    The groups mix tensors whose pass 1 accepts everything (they take the helper wave's second order), tensors whose pass 1 rejects
    (their own shuffle from the shared generator state) and one tensor of another seed (its own generator from the start)."""
    orders = {}
    mixed = 0
    for cs in of_metric(sc.shared_seed_cases(77, 78), metric).values():
        T = cs[0]["T"]
        if T not in orders:
            orders[T] = hb.scan_orders_device(77, T, 2)
        L = Launch(cs)
        L.run(orders=orders[T])
        L.check("shared orders")
        kinds = {("other seed" if c["seed"] != 77 else "p1 accepts" if all(v[3] for v in c.get("trace", ()) if v[0] == 1) else "p1 rejects") for c in cs}
        mixed += len(kinds) == 3
    assert mixed >= 6      # the three lists of more than two formats at T = 130 and 577


def expected_listed(L):
    T = L.T
    want = {}
    for b, c in enumerate(L.cs):
        last = len(c["formats"]) - 1
        fixed = c["fixed_before"][last]
        want[b] = b * T + np.flatnonzero(~fixed)
    return want


def check_listed(L, listed, n_listed):
    """listed[:n_listed] is a disjoint union of per-tensor segments, each ascending and equal to b·T + where(~fixed) of the plain scan
    before its last pass; nothing of a tensor that is done."""
    import torch

    torch.cuda.synchronize()
    n = int(n_listed.item())
    want = expected_listed(L)
    assert n == sum(v.size for v in want.values()), (L.cs[0]["name"], n)
    lst = listed[:n].cpu().numpy().astype(np.int64)
    segments = np.split(lst, np.flatnonzero(np.diff(lst // L.T)) + 1) if n else []
    owners = [int(s[0] // L.T) for s in segments]
    assert len(set(owners)) == len(owners), (L.cs[0]["name"], "a tensor's entries are not one segment")
    for s, b in zip(segments, owners):
        assert np.all(np.diff(s) > 0), (L.cs[b]["name"], "segment not ascending")
        assert np.array_equal(s, want[b]), (L.cs[b]["name"], s.size, want[b].size)
    for b, v in want.items():
        assert v.size == 0 or b in owners, L.cs[b]["name"]


@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("metric", ["mae", "pcc"])
def test_phases_and_listed(metric, shared):
    """Phase 1 (every pass but the last, then the last pass's candidates → listed), the list's contents, phase 2 (the last pass) — on the
    same full records."""
    import torch

    L_ = hb.lib()
    cases = sc.shared_seed_cases(77, 78) if shared else sc.own_seed_cases()
    orders = {}
    for cs in of_metric(cases, metric).values():
        T = cs[0]["T"]
        if shared and T not in orders:
            orders[T] = hb.scan_orders_device(77, T, 2)
        L = Launch(cs)
        listed = torch.full((L.count * T,), -1, dtype=torch.int32, device="cuda")
        nl = torch.zeros((1,), dtype=torch.int32, device="cuda")
        carry = torch.zeros((int(L_.mtq_scan_carry_bytes(L.count)),), dtype=torch.uint8, device="cuda")
        L.run(orders=orders.get(T), phase=1, listed=listed, n_listed=nl, carry=carry)
        check_listed(L, listed, nl)
        L.run(phase=2, carry=carry)
        L.check("phases")


@pytest.mark.parametrize("metric", ["mae", "pcc"])
def test_order_route_threshold(metric):
    """T = 32 768 keeps the visiting order in LDS, T = 32 769 in global scratch; with shared orders both run in global scratch."""
    for c in sc.order_route_cases(5):
        if c["metric"] != metric:
            continue
        L = Launch([c])
        L.run()
        L.check("own shuffles")
        L.maps.fill_(-1)
        L.run(orders=hb.scan_orders_device(5, c["T"], 1))
        L.check("shared orders")


def test_atol_walk():
    """greedy_atol on synthesized maxima: at thr and one ulp above it, a base maximum over thr, NaN in and out of the list."""
    seen = set()
    for cs in sc.grouped(sc.atol_cases(5)).values():
        L = Launch(cs)
        mask, formats, m, thr, n = L.args
        L.maps, L.status = hb.greedy_scan_device(L.recs, mask, formats, m, thr, n, L.seeds, counts_out=L.counts)
        L.check("atol")
        seen |= {(c["kind"], c["status"]) for c in cs}
    assert seen == {("mixed", 0), ("base_over", 0), ("nan_listed", 1), ("nan_unlisted", 0)}
