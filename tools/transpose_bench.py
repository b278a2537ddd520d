"""K1T (mtq_tile_stats_transposed) against the row-layout K1 (mtq_tile_stats_batched) on the same batches, mask 0xF, and against the
copy route on one tensor (x.T.contiguous(), K2 per format, torch reductions for pcc / mae / atol).  HIP events on the launch stream;
each figure is the median of REGIONS timed regions after a warm-up.  frac = algorithmic bytes read (2 B per bf16 / 4 B per float32
element) / time / 8 TB/s, as bench.py computes it.

    python tools/transpose_bench.py [REGIONS]
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from quantization_analysis_amd import hip_backend as hb  # noqa: E402

HBM_PEAK_GBS = 8000.0
REGIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
MASK = 0xF


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


def k1_pair(name, x):
    count, rows, cols = x.shape
    esz = x.element_size()
    elems = x.numel()
    row = timed(lambda: hb.tile_stats_batched(x, MASK))
    col = timed(lambda: hb.tile_stats_transposed(x, MASK))
    rec_bytes = count * hb.tiles_hw(rows, cols)[0] * hb.tiles_hw(rows, cols)[1] * hb.record_doubles(MASK) * 8
    out = {"batch": name, "elements": elems, "read_bytes": elems * esz, "record_bytes": rec_bytes}
    for k, ms in (("k1_rows", row), ("k1t", col)):
        gbs = elems * esz / (ms * 1e-3) / 1e9
        out[k] = {"ms": ms, "GBps_read": gbs, "frac": gbs / HBM_PEAK_GBS}
    out["k1t_over_k1"] = col / row
    return out


def copy_route(x2d):
    fmts = hb.mask_formats(MASK)

    def run():
        xt = x2d.T.contiguous()
        xf = xt.float()
        xm = xf - xf.mean()
        nx = torch.linalg.vector_norm(xm)
        cols = []
        for f in fmts:
            y = hb.quantize(xt, f)
            d = (xf - y).abs()
            ym = y - y.mean()
            cols.append(((xm * ym).sum() / (nx * torch.linalg.vector_norm(ym)), d.mean(), d.max()))
        return cols

    return timed(run)


def main():
    hb.require_gpu()
    torch.manual_seed(0)
    results = []
    x = (torch.randn((128, 4096, 4096), device="cuda") * 0.02).to(torch.bfloat16)
    results.append(k1_pair("128 x 4096x4096 bf16", x))
    del x
    torch.cuda.empty_cache()
    g = torch.randn((8, 14336, 4096), device="cuda") * 0.02
    x = g * torch.exp(1.5 * torch.randn_like(g))
    del g
    results.append(k1_pair("8 x 14336x4096 float32 (heavy tails)", x))
    del x
    torch.cuda.empty_cache()

    x2d = (torch.randn((4096, 14336), device="cuda") * 0.02).to(torch.bfloat16)
    k1t = timed(lambda: hb.tile_stats_transposed(x2d, MASK))
    cr = copy_route(x2d)
    elems = x2d.numel()
    nf = len(hb.mask_formats(MASK))
    results.append({"tensor": "4096x14336 bf16", "elements": elems,
                    "k1t": {"ms": k1t, "bytes": elems * 2 + hb.tiles_hw(14336, 4096)[0] * hb.tiles_hw(14336, 4096)[1] * hb.record_doubles(MASK) * 8,
                            "frac": elems * 2 / (k1t * 1e-3) / 1e9 / HBM_PEAK_GBS},
                    "copy_route": {"ms": cr, "bytes": elems * (4 + 12 * nf), "note": "transpose copy 4 B/elem, per format K2 6 B + reductions 6 B"},
                    "copy_route_over_k1t": cr / k1t})
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
