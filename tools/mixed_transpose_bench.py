"""The mixed-tile searches over the transposed layout (params["layout"] = "transpose") on the hip backend:
  * K3T (mtq_apply_assignment_transposed) against K3 on one 4096×14336 bf16 tensor with a mixed map (HIP events; effective bandwidth =
    2 B read + 4 B written per element);
  * K1T against the row-layout K1 on 128 × 4096² bf16, mask 0xF (HIP events);
  * GreedyPipeline(layout="transpose") against the row layout on the same 128 × 4096² bf16 batch (pcc >= 0.999, seed 123, the device
    scan), the step time of run_steps as bench.py times it, beside K1T alone;
  * ThresholdPipeline(layout="transpose") against the row layout on a few float32 shapes (pcc >= 0.999, run_batches).
Each figure is the median of REGIONS timed regions after a warm-up.

    python tools/mixed_transpose_bench.py [REGIONS]
"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from quantization_analysis_amd import hip_backend as hb  # noqa: E402

REGIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
MASK = 0xF
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2"]


def timed(fn, warm=2, regions=REGIONS):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def k3_pair():
    g = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.randn((4096, 14336), device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    rng = np.random.default_rng(7)
    map_rows = torch.from_numpy(rng.integers(0, 4, size=hb.tiles_hw(4096, 14336)).astype(np.int8)).cuda()
    map_t = torch.from_numpy(rng.integers(0, 4, size=hb.tiles_hw(14336, 4096)).astype(np.int8)).cuda()
    y = torch.empty((4096, 14336), dtype=torch.float32, device="cuda")
    y3 = y.view(1, 4096, 14336)
    row = timed(lambda: hb.apply_assignment(x, map_rows, out=y))
    col = timed(lambda: hb.apply_assignment_transposed(x, map_t, out=y3))
    moved = x.numel() * 6
    return {"shape": [4096, 14336], "k3_ms": row, "k3t_ms": col, "k3_TBps": moved / (row * 1e-3) / 1e12,
            "k3t_TBps": moved / (col * 1e-3) / 1e12, "k3t_over_k3": col / row}


def k1_pair():
    x = (torch.randn((128, 4096, 4096), device="cuda") * 0.02).to(torch.bfloat16)
    row = timed(lambda: hb.tile_stats_batched(x, MASK))
    col = timed(lambda: hb.tile_stats_transposed(x, MASK))
    tiles = 128 * 128 * 128
    del x
    torch.cuda.empty_cache()
    return {"batch": "128 x 4096^2 bf16", "k1_ms": row, "k1t_ms": col, "k1t_Gtiles_per_s": tiles / (col * 1e-3) / 1e9, "k1t_over_k1": col / row}


def wall(fn, steps: int = 5, regions=REGIONS):
    """Median wall time of `steps` calls, per call, synchronised (ms)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _s in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / steps)
    ts.sort()
    return ts[len(ts) // 2]


def greedy_pipeline_pair():
    from quantization_analysis_amd.pipeline import GreedyPipeline

    x = (torch.randn((128, 4096, 4096), device="cuda") * 0.02).to(torch.bfloat16)
    out = {"batch": "128 x 4096^2 bf16, pcc >= 0.999, seed 123", "tiles": 128 * 128 * 128}
    for layout in ("rows", "transpose"):
        with GreedyPipeline(FORMATS, "pcc", 0.999, 123, chunk=1 << 30, layout=layout) as pipe:
            pipe.reserve(x)
            step = wall(lambda: pipe.run_steps([x, x, x]), steps=1) / 3
            out[f"{layout}_step_ms"] = step
            out[f"{layout}_Gtiles_per_s"] = out["tiles"] / (step * 1e-3) / 1e9
            out[f"{layout}_device_scan"] = pipe._use_device_scan(128 * 128)
    out["k1t_alone_ms"] = timed(lambda: hb.tile_stats_transposed(x, 0xE))
    out["transpose_step_over_k1t"] = out["transpose_step_ms"] / out["k1t_alone_ms"]
    del x
    torch.cuda.empty_cache()
    return out


def threshold_pipeline_pair():
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    shapes = [(8, 4096, 14336), (8, 14336, 4096), (16, 4096, 4096), (4, 1000, 3000)]
    out = []
    for count, rows, cols in shapes:
        x = torch.randn((count, rows, cols), device="cuda") * 0.02
        row = {"batch": f"{count} x {rows}x{cols} float32"}
        for layout in ("rows", "transpose"):
            with ThresholdPipeline(FORMATS, "pcc", 0.999, chunk=1 << 30, layout=layout) as pipe:
                row[f"{layout}_ms"] = wall(lambda: pipe.run_batches([x]))
        out.append(row)
        del x
    torch.cuda.empty_cache()
    return out


def main():
    hb.require_gpu()
    print(json.dumps({"k3": k3_pair(), "k1": k1_pair(), "greedy_pipeline": greedy_pipeline_pair(), "threshold_pipeline": threshold_pipeline_pair(),
                      "regions": REGIONS}, indent=1))


if __name__ == "__main__":
    main()
