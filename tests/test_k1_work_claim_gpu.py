"""K1's work claim on the device: every unit computed exactly once at every grid geometry (tests/k1_claim_cases.py has the rule: records
go into buffers filled with a NaN pattern no kernel writes, and must come back without it and with the oracle's bits).

(a) the default geometry at the size bench.py runs, through every route that launches K1; (b) the regime borders of this device;
(c) every geometry switch, each in a fresh child process (the library reads its switches once); (d) a walk of four rounds through
the ring of counter slots, over both ways a slot is zeroed again; (e) the streamed driver's record slots, refilled with the pattern
between steps of DIFFERENT tensors.  The host side of the same arithmetic is tests/test_k1_grid_host.py."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mtq_oracle as orc  # noqa: E402
from quantization_analysis_amd import hip_backend as hb  # noqa: E402
from tests import k1_claim_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
REGIMES = {"resident", "quota", "oversubscribed"}


def _regimes(log, kind):
    return {e["regime"] for e in log if e["kind"] == kc.KIND_NAME[kind]}


# ------------------------------------------------------------------------------------------------------------------ (a)
def test_bench_scale_bf16_every_route():
    """128 x 4096² bf16 (524 288 units: 32 832 blocks on 256 CUs, the oversubscribed regime bench.py runs) from 4 distinct tensors in
    a shuffled order, through the whole-record launch with and without the bf16 slot, the partial launch, and the two-launch form
    the streamed driver uses (the launch zeroes its own counters): all 128 record blocks against the oracle."""
    case = kc.uniform_case(kc.BF16, 128 * 128 * 32, 11, force=(128, 128, 32, 4))
    assert tuple(case.x.shape) == (128, 4096, 4096) and case.x.dtype == torch.bfloat16
    assert hb.k1_regime(kc.BF16, case.total, kc.cus()) == "oversubscribed"
    log = []
    fails = kc.run_case(case, ("batched_f", "batched_e", "partial", "begin_end"), log)
    assert not fails, fails
    assert len(log) == 4 and hb.work_counters_nonzero() == 0


def test_bench_scale_float32_direct_kernel():
    """16 x (3072 x 8192) float32 = 393 216 tiles from 2 distinct tensors: the direct kernel beyond its resident grid."""
    case = kc.uniform_case(kc.DIRECT, 16 * 96 * 256, 12, force=(16, 96, 256, 2), trim=(0, 0))
    assert tuple(case.x.shape) == (16, 3072, 8192) and case.x.dtype == torch.float32
    assert hb.k1_regime(kc.DIRECT, case.total, kc.cus()) == "oversubscribed"
    fails = kc.run_case(case, ("batched_f",), [])
    assert not fails, fails
    assert hb.work_counters_nonzero() == 0


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_regime_borders_of_this_device():
    """The largest all-resident total and the next one, the largest total on the resident grid with a quota and the next one, and one
    below / above a multiple of 64 x W x quota, for both kernels and for ragged batches of the same tile counts."""
    log = []
    fails = kc.border_cases(log)
    assert not fails, fails
    for kind in (kc.BF16, kc.DIRECT):
        assert _regimes(log, kind) == REGIMES, (kind, log)
    assert sum(e["route"] == "ragged" for e in log) == 6 and {e["regime"] for e in log if e["route"] == "ragged"} == REGIMES
    assert hb.work_counters_nonzero() == 0


# ------------------------------------------------------------------------------------------------------------------ (c)
# Measured on an MI355X: 2.6 - 3.1 s of wall time per child, 0.6 - 1.0 s of it the cases themselves (the slowest: MTQ_K1_UNITS_PER_WAVE=64,
# whose borders lie at 3.3 M tiles), the rest the interpreter and the library coming up.  The limit is a hundred times that: a child
# that needs it hangs, and a slow, busy host does not trip it.
CHILD_SECONDS_MEASURED = 3.1
CHILD_TIMEOUT = 300
SWITCHES = [{"MTQ_K1_UNITS_PER_WAVE": u, **({"MTQ_K1_WAVES": w} if w else {})} for u in ("0", "1", "3", "64") for w in (None, "1", "5")] + \
           [{"MTQ_K1_LDS_PAD": "4096"}, {"MTQ_LISTED_DIRECT": "1"}, {"MTQ_LISTED_WAVES": "1"}]
OWN = ("MTQ_K1_UNITS_PER_WAVE", "MTQ_K1_WAVES", "MTQ_K1_LDS_PAD", "MTQ_LISTED_DIRECT", "MTQ_LISTED_WAVES")
_children = {"stopped": None, "seen": {kc.BF16: set(), kc.DIRECT: set()}, "ran": 0}


def _reachable(kind: int, n_cu: int, switches: dict) -> set:
    """The regimes that geometry HAS, from the regimes' definitions: without a quota waves never retire (resident / persistent); a
    quota regime on the resident grid exists only where a grid of one block per group less than the resident one, at `quota` claims
    per wave, holds more units than there are resident waves."""
    W = 2
    wps = int(switches.get("MTQ_K1_WAVES", 3)) if kind == kc.BF16 else 3
    q = int(switches.get("MTQ_K1_UNITS_PER_WAVE", 8)) * (16 if kind == kc.DIRECT else 1)
    mb = n_cu * wps * 4 // W
    if q == 0:
        return {"resident", "persistent"}
    return {"resident", "oversubscribed"} | ({"quota"} if (mb // 64 - 1) * 64 * W * q > mb * W else set())


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: ",".join(f"{k[4:]}={v}" for k, v in s.items()))
def test_geometry_switches_in_fresh_processes(switches):
    """tests/k1_claim_cases.py in a child of its own per switch combination: its borders, its listed completions.  The child must
    report no failure, a clean ring, and every regime its geometry has for both kernels - a child that tested nothing fails."""
    if _children["stopped"]:
        pytest.fail(f"not started: an earlier child ended by signal or timeout ({_children['stopped']})")
    env = {k: v for k, v in os.environ.items() if k not in OWN}
    env.update(switches)
    try:
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "k1_claim_cases.py")], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        _children["stopped"] = f"{switches}: timeout"
        raise
    if r.returncode < 0:
        _children["stopped"] = f"{switches}: signal {-r.returncode}"
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1].startswith("{"), (r.returncode, r.stderr[-3000:])
    rep = json.loads(lines[-1])
    print(f"child {switches}: {rep['seconds']} s, {len(rep['launches'])} K1 launches, {rep['listed_launches']} listed launches")
    assert rep["failures"] == [] and r.returncode == 0, rep["failures"]
    assert rep["counters_nonzero"] == 0
    assert rep["listed_launches"] == 4 * 4 * 2
    for kind in (kc.BF16, kc.DIRECT):
        seen = _regimes(rep["launches"], kind)
        assert seen == _reachable(kind, rep["cus"], switches), (kind, seen, rep["launches"])
        _children["seen"][kind] |= seen
    _children["ran"] += 1


def test_switch_children_reached_every_regime():
    assert _children["ran"] == len(SWITCHES) and not _children["stopped"], _children
    for kind in (kc.BF16, kc.DIRECT):
        assert _children["seen"][kind] == REGIMES | {"persistent"}, _children["seen"]


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_ring_walk_over_both_resets():
    """640 consecutive launches (512 of them take a counter slot: four rounds of the ring of 128) over 4 streams, rotating over the
    bf16 whole-record launch (its follow-up kernel zeroes the slot), the two-launch form (the launch's last wave does), the direct kernel, a ragged batch and K1T (which only stamps): a
    counter left over by any of them meets its slot's next user one round later.  Every launch is checked, and the ring is clean."""
    bf = kc.uniform_case(kc.BF16, 3 * 5 * 41, 21)          # 615 units: 308 blocks, every group in use
    f32 = kc.uniform_case(kc.DIRECT, 2 * 3 * 61, 22)
    rag = kc.ragged_case(333, 23)
    xt = kc._rand(24, (96, 160), False)
    want_t = torch.from_numpy(orc.tile_stats(np.ascontiguousarray(xt.cpu().numpy().T), ALL).view(np.int64)).cuda()
    plan = [(bf, "batched_e"), (bf, "begin_end"), (f32, "batched_f"), (rag, "ragged"), (None, "transposed")]
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    fails, pending, launches = [], [], 5 * 128

    def drain():
        torch.cuda.synchronize()
        for case, args in pending:
            if case is None:
                got = args.view(-1, 22).view(torch.int64)
                if bool((got == kc.SENTINEL).any()) or not torch.equal(got, want_t):
                    fails.append("transposed records differ from the oracle")
            else:
                fails.extend(case.check(*args))
        pending.clear()

    for i in range(launches):
        case, route = plan[i % len(plan)]
        with torch.cuda.stream(streams[i % len(streams)]):
            if case is None:
                out = kc.sentinel_filled((want_t.shape[0], 22))
                hb.tile_stats_transposed(xt, 0xF, out=out[None])
                pending.append((None, out))
            else:
                pending.append((case, kc.launch(case, route)))
        if len(pending) == 64:
            drain()
    drain()
    assert not fails, fails[:8]
    assert hb.work_counters_nonzero() == 0


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("scan", ["device", "host"])
def test_pipeline_slots_hold_no_stale_records(scan):
    """GreedyPipeline over 4 steps of 96 x 1024² bf16 (24 576 units in one K1 launch: oversubscribed), every step made of tensors no
    earlier step held, every slot's record buffer refilled with the pattern between steps: a unit K1 skipped cannot show an earlier
    step's (then wrong) or this step's (then right) answer.  Maps, counts and columns of every tensor of every step against the oracle."""
    from quantization_analysis_amd.pipeline import GreedyPipeline

    count, thr, seed = 96, 0.999, 4242
    assert hb.k1_regime(kc.BF16, count * 32 * 8, kc.cus()) == "oversubscribed"
    steps = []
    for s in range(4):
        dist = [kc._rand(500 + 10 * s + d, (1024, 1024), True) for d in range(2)]
        kc._spoil(dist[0], 0, 0, 128, 0)                   # the first unit of the batch …
        kc._spoil(dist[1], 31, 896, 128, int(s == 3))      # … and its last go through the literal fix-up (step 3: a 2e18 element)
        order = np.random.default_rng(s).integers(0, 2, size=count)
        order[0], order[-1] = 0, 1
        want = []
        for d in dist:
            x = d.float().cpu().numpy()
            a, counts, st = orc.greedy(x, ALL, "pcc", thr, seed)
            want.append((a, counts, orc.columns_from_stats(st["stats"], orc.mask_slots(0xF), a, x.size)))
        steps.append((torch.stack(dist)[torch.from_numpy(order).cuda()].contiguous(), order, want))

    def refill(pipe):
        torch.cuda.synchronize()
        bufs = [b["dev"] for b in pipe._devbufs.values()] + [t for v in pipe._bufs.values() for t in v[1:3]]
        assert len(bufs) >= pipe.SLOTS
        for t in bufs:
            t.view(torch.int64).fill_(kc.SENTINEL)
        torch.cuda.synchronize()

    with GreedyPipeline(ALL, "pcc", thr, seed, chunk=count, workers=4, scan=scan) as pipe:
        assert pipe.device_scan == (scan == "device")
        assert (pipe.lazy_plan(steps[0][0]) is not None) == (scan == "device")
        pipe.reserve(steps[0][0])
        for s, (xs, order, want) in enumerate(steps):
            refill(pipe)
            res = pipe.run(xs)
            assert [r.index for r in res] == list(range(count))
            for i, r in enumerate(res):
                a, counts, (pcc, mae, atol) = want[order[i]]
                assert np.array_equal(r.assignment, a) and r.counts == counts, (scan, s, i)
                assert abs(r.pcc - pcc) <= 1e-13 and abs(r.mae - mae) <= 1e-13 * max(mae, 1e-30) + 1e-18 and r.atol == atol, (scan, s, i)
    assert hb.work_counters_nonzero() == 0
