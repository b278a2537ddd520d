"""What the streamed drivers share: the result type, the K1 timing record, the CPU budget of a rank, the host-scan task and the columns
from seven sums (pipeline.py re-exports these; GreedyPipeline is in pipeline_greedy.py, ThresholdPipeline in pipeline_threshold.py)."""
from __future__ import annotations

import concurrent.futures as cf
import contextlib
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import hip_backend as hb
from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS, mixed_tile_total_bytes
from .settings import settings


@dataclass
class TensorResult:
    index: int
    assignment: np.ndarray  # int8 (tiles_h, tiles_w)
    counts: dict
    tile_bytes: float
    pcc: float
    mae: float
    atol: float
    metric_value: float
    pure: dict | None = None    # format name → (pcc, mae, atol) of the whole tensor in that one format (the `none` rows of wq), on request
    sums: object = field(default=None, repr=False, compare=False)   # Σx, Σx², Σy, Σy², Σxy, Σ|d| of the map (an owned copy)


@dataclass
class KernelTiming:
    launches: int = 0
    kernel_ms: float = 0.0      # Σ of HIP-event durations around the K1 launches
    tiles: int = 0              # Σ tiles processed by those launches
    events: list = field(default_factory=list)

    def drain(self) -> None:
        for e0, e1, tiles in self.events:
            e1.synchronize()
            self.kernel_ms += e0.elapsed_time(e1)
            self.tiles += tiles
            self.launches += 1
        self.events.clear()


def cpu_budget() -> int:
    """Hardware threads this process may really use: the cgroup CPU quota when there is one (a gpurun box shows 256
    hardware threads but runs under a 16-CPU quota; exceeding a CFS quota stalls every thread of the job for the rest of
    the 100 ms period), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def default_workers() -> int:
    """Scan threads per rank: the rank's share of the CPU budget (the driver's own threads mostly sleep), at most 32;
    MTQ_SCAN_WORKERS overrides."""
    if settings().scan_workers is not None:
        return settings().scan_workers
    local = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    return max(4, min(32, cpu_budget() // max(local, 1)))


def _scan_chunk(first, stats, mask, tiles_hw, numel, tile_formats, metric, threshold, seeds, n_threads) -> list[TensorResult]:
    """The searches of one chunk of tensors: a single GIL-free C call fanning out over n_threads host threads."""
    maps, counts, outs = hb.greedy_run_batch(stats, mask, tile_formats, metric, threshold, float(numel), seeds, n_threads)
    k = {"pcc": 0, "mae": 1, "atol": 2}[metric]
    res = []
    for j in range(maps.shape[0]):
        c = {f: int(counts[j, i]) for i, f in enumerate(MIXED_TILE_FORMATS)}
        res.append(TensorResult(first + j, maps[j].reshape(tiles_hw), c, mixed_tile_total_bytes(c), float(outs[j, 0]), float(outs[j, 1]),
                                float(outs[j, 2]), float(outs[j, k]), sums=outs[j, 3:9].copy()))
    return res


def _sleep_until(event, tick: float = 1e-4) -> None:
    """Wait for a HIP event without burning the core: hipEventSynchronize spins on this runtime even for events created with the
    blocking flag (the driver thread showed 100 % CPU while 'waiting'), so the event is polled between short sleeps.  The pipeline
    has a whole step of slack on this wait (several record slots)."""
    import time

    while not event.query():
        time.sleep(tick)


def _when_landed(event, fn, *args):
    """Chunk task of the streamed driver: sleep until the chunk's records are on the host (a blocking HIP event), then scan."""
    event.synchronize()
    return fn(*args)


def columns_from_sums_batch(sums: np.ndarray, n) -> np.ndarray:
    """mtq_columns_from_sums for many tensors at once: sums [count, 7] (Σx, Σx², Σy, Σy², Σxy, Σ|d|, max|d|) → [count, 3]
    pcc, mae, atol — the same double operations in the same order (metrics.py:6-16 as moments), element-wise in NumPy.  n: the tensors'
    element count, one number or one per tensor."""
    n = np.asarray(n, dtype=np.float64)
    sx, sx2, sy, sy2, sxy, sab, mx = (sums[:, i] for i in range(7))
    mean_x, mean_y = sx / n, sy / n
    am2 = np.maximum(sx2 - n * mean_x * mean_x, 0.0)
    bm2 = np.maximum(sy2 - n * mean_y * mean_y, 0.0)
    denom = np.sqrt(am2 * bm2)
    with np.errstate(all="ignore"):
        pcc = np.where(denom == 0.0, np.where(sab == 0.0, 1.0, 0.0), (sxy - n * mean_x * mean_y) / denom)
        mae = np.where(n != 0.0, sab / n, 0.0)
    return np.stack([pcc, mae, mx], axis=1)


# The pcc column's contract (DESIGN §2 "Float columns"): within PCC_F64_TOL of a float64 Pearson of (x, y) wherever Σx² and Σy² lie in
# the float32-safe range of csrc/mtq_decide.hpp.  The moment form above meets it unless the products K1 summed were rounded to float32
# (float32 storage: |fl(x·x) − x²| <= 2^-24·x²) and the tensor is offset: Σx² − n·mean² then leaves those rounding errors standing
# against a small variance.  To first order |Δpcc| <= 2^-24·(√(κx·κy) + (κx + κy)/2), κx = Σx²/am2, κy = Σy²/bm2 — the argument of
# pcc_moment_near applied to the whole tensor.  Where that exceeds the tolerance, centred_pcc recomputes the column from x and y.
PCC_F64_TOL = 2.5e-7
SUM_SQ_LO, SUM_SQ_HI = 2.0 ** -92, 2.0 ** 124
CENTRED_CHUNK = 1 << 22   # elements per float64 chunk of centred_pcc


def moment_pcc_gate(sums: np.ndarray, n, float32_storage: bool) -> np.ndarray:
    """bool [count]: is the moment-form pcc of each tensor (sums [count, >=4]: Σx, Σx², Σy, Σy², ...) possibly more than PCC_F64_TOL
    from a float64 Pearson?  Never for bf16 storage (its products with every format's y are exact in float32) nor outside the
    float32-safe range (those tensors keep their moment columns); always where am2 or bm2 is not positive."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, np.shape(sums)[-1])
    if not float32_storage:
        return np.zeros(sums.shape[0], dtype=bool)
    n = np.asarray(n, dtype=np.float64)
    sx, sx2, sy, sy2 = (sums[:, i] for i in range(4))
    mean_x, mean_y = sx / n, sy / n
    am2 = sx2 - n * mean_x * mean_x
    bm2 = sy2 - n * mean_y * mean_y
    in_range = (sx2 >= SUM_SQ_LO) & (sx2 <= SUM_SQ_HI) & (sy2 >= SUM_SQ_LO) & (sy2 <= SUM_SQ_HI)
    with np.errstate(all="ignore"):
        kx, ky = sx2 / am2, sy2 / bm2
        bound = 2.0 ** -24 * (np.sqrt(kx * ky) + 0.5 * (kx + ky))
        ok = (am2 > 0.0) & (bm2 > 0.0) & (bound <= PCC_F64_TOL)
    return in_range & ~ok


def _is_float32(x) -> bool:
    return str(x.dtype) in ("float32", "torch.float32")


def centred_pcc(x, y, sums, n) -> float:
    """Pearson r of the first n elements of the flattens of x and y (NumPy arrays or torch tensors: a padded vector's zeros trail) from
    float64 Σ(x−x̄)², Σ(y−ȳ)², Σ(x−x̄)(y−ȳ) around the means of the record sums, in chunks of CENTRED_CHUNK elements; the zero-denominator
    rule of the moment form (1 when Σ|x−y| = 0, else 0)."""
    n = int(n)
    mx, my = float(sums[0]) / n, float(sums[2]) / n
    xf, yf = x.reshape(-1), y.reshape(-1)
    cxx = cyy = cxy = 0.0
    for i in range(0, n, CENTRED_CHUNK):
        j = min(n, i + CENTRED_CHUNK)
        if hasattr(xf, "double"):
            a, b = xf[i:j].double() - mx, yf[i:j].double() - my
            cxx += float(a.dot(a)); cyy += float(b.dot(b)); cxy += float(a.dot(b))
        else:
            a, b = np.asarray(xf[i:j], dtype=np.float64) - mx, np.asarray(yf[i:j], dtype=np.float64) - my
            cxx += float(a @ a); cyy += float(b @ b); cxy += float(a @ b)
    denom = float(np.sqrt(cxx * cyy))
    if denom == 0.0:
        return 1.0 if float(sums[5]) == 0.0 else 0.0
    return cxy / denom


def gated_pcc(pcc: float, sums, n, x, y_of) -> float:
    """The pcc column of one tensor: the moment value `pcc`, or — where moment_pcc_gate fires for x's storage — centred_pcc of x and
    y_of() (y in x's layout, only made then).  Every route that reports a pcc column passes it through here."""
    if not moment_pcc_gate(np.asarray(sums, dtype=np.float64)[None, :6], float(n), _is_float32(x))[0]:
        return float(pcc)
    return centred_pcc(x, y_of(), sums, n)


def gated_columns(cols: np.ndarray, sums: np.ndarray, n, xs, y_of) -> np.ndarray:
    """columns_from_sums_batch's [count, 3] with each tensor's pcc through gated_pcc: xs[j] the tensor's x, y_of(j) its y."""
    count = cols.shape[0]
    if count == 0:
        return cols
    n = np.broadcast_to(np.asarray(n, dtype=np.float64), (count,))
    for j in np.flatnonzero(moment_pcc_gate(sums[:count, :6], n, True)):
        if _is_float32(xs[j]):   # a ragged group may mix storage types
            cols[j, 0] = centred_pcc(xs[j], y_of(j), sums[j], n[j])
    return cols
