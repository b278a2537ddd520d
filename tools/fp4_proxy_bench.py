"""FP4P timing: mtq_fp4_proxy_sums (both proxies, mask 0b11) on one 4096x4096 bf16 and one 14336x4096 float32 tensor, HIP events on the
launch stream (median of `reps`), against the 8 TB/s read roofline; beside it K1 (mtq_tile_stats, mask 0xF) on the same 4096x4096 bf16
tensor.  Buffers are allocated before timing.  The VALU count per element is tools/isa_mix.py's on the listing of csrc/mtq_fp4_proxy.hip
(hipcc -S --cuda-device-only), divided by the elements one loop iteration handles (8 bf16 / 4 float32).
usage: python tools/fp4_proxy_bench.py [reps]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from quantization_analysis_amd import hip_backend as hb  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
hb.require_gpu()


def median_ms(fn) -> float:
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


g = torch.Generator(device="cuda")
g.manual_seed(0)
out = []
for rows, cols, dtype in [(4096, 4096, torch.bfloat16), (14336, 4096, torch.float32)]:
    x = (torch.randn((rows, cols), generator=g, device="cuda") * 0.02).to(dtype)
    need = int(hb.lib().mtq_fp4_proxy_scratch_doubles(1, rows, cols))
    scratch = torch.empty(need, dtype=torch.float64, device="cuda")
    sums = torch.zeros((1, 2, 7), dtype=torch.float64, device="cuda")
    ms = median_ms(lambda: hb.fp4_proxy_sums(x, hb.PROXY_FORMATS, out=sums, scratch=scratch))
    nbytes = rows * cols * x.element_size()
    row = {"kernel": "mtq_fp4_proxy_sums", "shape": [rows, cols], "dtype": str(dtype).split(".")[-1], "median_ms": round(ms, 4),
           "gelem_per_s": round(rows * cols / ms / 1e6, 1), "read_gb_per_s": round(nbytes / ms / 1e6, 1), "roofline_frac": round(nbytes / ms / 1e6 / 8000, 4)}
    if dtype == torch.bfloat16:
        stats = hb.tile_stats(x, 0xF)
        row["k1_mask_0xF_median_ms"] = round(median_ms(lambda: hb.tile_stats(x, 0xF, out=stats)), 4)
        row["ratio_to_k1"] = round(ms / row["k1_mask_0xF_median_ms"], 2)
    out.append(row)
    print(json.dumps(row), flush=True)
