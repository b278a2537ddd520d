"""mtq_packed_matmul (the product with a packed k × n matrix) and the transposed pack / unpack, timed by tools/packed_linear_bench.py's
method: device events after a warm-up, --rounds rounds of a window each, the sides alternated in one process, the C entries called
directly, the weights rotated over --cold-mb of copies.

  matmul  : P (k × n) in {4096 × 4096, 4096 × 14336, 14336 × 4096}, m in {1, 16, 256, 4096}, an all-bfp8, an all-bfp4 and a greedy map.
            Three sides: mtq_packed_matmul on P's stream; mtq_packed_linear (the block kernel) on the n × k stream of Pᵀ under the
            transposed map (the same tile counts, so the same bytes); torch.matmul on the unpacked bf16 P̂.  Before timing, the bit
            contract is checked: mtq_packed_matmul against mtq_packed_linear on the all-bf16 packing of unpack(P̂)ᵀ.
            `matmul/block-min` is the new kernel's median over the block kernel's MINIMUM of the same run; `spread` is the block
            kernel's median over its minimum (the run's own noise).
  pack    : mtq_pack_tiles_transposed / mtq_unpack_tiles_transposed on the stored n × k weight against mtq_pack_tiles /
            mtq_unpack_tiles on the same tensor under the transposed map; bytes moved over time.

  python tools/packed_matmul_bench.py [--rounds 5] [--window-ms 30] [--out profiles/packed_matmul.txt] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb
from tools.packed_linear_bench import calibrate, greedy_map, window_ms


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=30.0)
    p.add_argument("--cold-mb", type=float, default=640.0, help="rotate over copies of the weight worth this many MB")
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--shapes", default="4096x4096,4096x14336,14336x4096", help="k x n of the packed matrix, comma separated")
    p.add_argument("--ms", default="1,16,256,4096")
    p.add_argument("--maps", default="bfp8,bfp4,greedy")
    p.add_argument("--skip-pack", action="store_true", help="skip the pack / unpack timings")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    if not hb.has_packed_matmul():
        raise hb.MtqError("this build of libmtq_hip.so lacks mtq_packed_matmul")
    rows, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# mtq_packed_matmul on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"weights rotated over {args.cold_mb:.0f} MB; HBM figure {args.hbm_tbs} TB/s")
    stream = torch.cuda.current_stream().cuda_stream
    for shape in args.shapes.split(","):
        k, n = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + k)
        pm = (torch.randn((k, n), generator=g, device="cuda") * 0.02).to(torch.bfloat16)      # P, k × n
        w = pm.t().contiguous()                                                               # W = Pᵀ, n × k as a linear layer stores it
        th, tw = hb.tiles_hw(k, n)
        maps = {"bfp8": lambda: np.full((th, tw), 1, dtype=np.int8), "bfp4": lambda: np.full((th, tw), 2, dtype=np.int8), "greedy": lambda: greedy_map(pm)}
        for name in args.maps.split(","):
            amap = maps[name]()
            counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
            tp = hb.PackedTables.on_device(amap)                                              # over P's grid
            tl = hb.PackedTables.on_device(np.ascontiguousarray(amap.T))                      # over W's grid: the same counts
            assert tp.nbytes == tl.nbytes
            dp = hb.pack_tiles_transposed(w, tp)                                              # P's stream, from W read in place
            assert torch.equal(dp, hb.pack_tiles(pm, tp))
            dl = hb.pack_tiles(w, tl)                                                         # W's row-layout stream: the block kernel's side
            pq = hb.unpack_tiles(dp, tp, k, n, dtype=torch.bfloat16)                          # P̂ bf16, k × n
            if not args.skip_pack:
                y16 = torch.empty((n, k), dtype=torch.bfloat16, device="cuda")
                sides = (("pack_transposed", lambda i: hb.pack_tiles_transposed(w, tp, out=dp), 2 * n * k + tp.nbytes),
                         ("pack_rows", lambda i: hb.pack_tiles(w, tl, out=dl), 2 * n * k + tl.nbytes),
                         ("unpack_transposed_bf16", lambda i: hb.unpack_tiles_transposed(dp, tp, n, k, dtype=torch.bfloat16, out=y16), tp.nbytes + 2 * n * k),
                         ("unpack_rows_bf16", lambda i: hb.unpack_tiles(dl, tl, n, k, dtype=torch.bfloat16, out=y16), tl.nbytes + 2 * n * k))
                iters = [calibrate(fn, args.window_ms) for _w, fn, _b in sides]
                ts = [[] for _ in sides]
                for _ in range(args.rounds):
                    for j, (_w, fn, _b) in enumerate(sides):
                        ts[j].append(window_ms(fn, iters[j]))
                for j, (what, _fn, moved) in enumerate(sides):
                    med = statistics.median(ts[j])
                    rows.append({"what": what, "n": n, "k": k, "map": name, "counts": counts, "ms_median": med, "ms_min": min(ts[j]), "bytes": moved,
                                 "tbs": moved / med / 1e9})
                    say(f"{what:22s} W {n}x{k} map={name:6s} counts={counts} {med * 1e3:9.1f} us (min {min(ts[j]) * 1e3:9.1f})  "
                        f"{moved / med / 1e9:6.3f} TB/s = {100 * moved / med / 1e9 / args.hbm_tbs:5.1f}% of {args.hbm_tbs} TB/s")
                del y16
            # the contract pair: the all-bf16 row-layout packing of unpack(P̂)ᵀ
            tb = hb.PackedTables.on_device(np.zeros(hb.tiles_hw(n, k), dtype=np.int8))
            db = hb.pack_tiles(pq.t().contiguous(), tb)
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / tp.nbytes)))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (2 * n * k))))
            dps = [dp] + [dp.clone() for _ in range(copies_p - 1)]
            dls = [dl] + [dl.clone() for _ in range(copies_p - 1)]
            pqs = [pq] + [pq.clone() for _ in range(copies_w - 1)]
            for m in (int(v) for v in args.ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                ya, yb, ym = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(3))
                hb.packed_matmul(x, dp, tp, n, out_dtype=torch.bfloat16, out=ya)               # the wrappers' checks, once
                hb.packed_linear(x, db, tb, n, out_dtype=torch.bfloat16, out=yb)
                same = bool(torch.equal(ya.view(torch.int16), yb.view(torch.int16)))
                e_mm, e_lin = hb._entry("mtq_packed_matmul"), hb._entry("mtq_packed_linear")
                c_mm = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tp.nbytes, tp.map_ptr, tp.offsets_ptr, n, None, ya.data_ptr(), hb.DTYPE_BF16, n,
                         stream) for d in dps]
                c_lin = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tl.nbytes, tl.map_ptr, tl.offsets_ptr, n, None, yb.data_ptr(), hb.DTYPE_BF16, n,
                          stream) for d in dls]

                def f_mm(i):
                    hb.check(e_mm(*c_mm[i % copies_p]))

                def f_lin(i):
                    hb.check(e_lin(*c_lin[i % copies_p]))

                def f_torch(i):
                    torch.matmul(x, pqs[i % copies_w], out=ym)

                fns = (f_mm, f_lin, f_torch)
                iters = [calibrate(fn, args.window_ms) for fn in fns]
                ts = [[], [], []]
                for _ in range(args.rounds):
                    for j, fn in enumerate(fns):
                        ts[j].append(window_ms(fn, iters[j]))
                f_mm(0)
                f_torch(0)
                err = float((ya.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                med = [statistics.median(t) for t in ts]
                mn = [min(t) for t in ts]
                flop = 2.0 * m * n * k
                rows.append({"what": "packed_matmul", "k": k, "n": n, "m": m, "map": name, "counts": counts, "matmul_ms_median": med[0],
                             "matmul_ms_min": mn[0], "block_ms_median": med[1], "block_ms_min": mn[1], "torch_ms_median": med[2], "torch_ms_min": mn[2],
                             "matmul_over_block_min": med[0] / mn[1], "block_spread": med[1] / mn[1], "matmul_over_torch": med[0] / med[2],
                             "stream_gbs": tp.nbytes / med[0] / 1e6, "matmul_tflops": flop / med[0] / 1e9, "block_tflops": flop / med[1] / 1e9,
                             "torch_tflops": flop / med[2] / 1e9, "contract_bits_equal": same, "max_rel_diff_torch": err})
                say(f"matmul P {k}x{n} m={m:5d} map={name:6s} new {med[0] * 1e3:9.1f} us (min {mn[0] * 1e3:9.1f}, {tp.nbytes / med[0] / 1e6:7.1f} GB/s of stream) "
                    f"block {med[1] * 1e3:9.1f} us (min {mn[1] * 1e3:9.1f}) torch {med[2] * 1e3:9.1f} us (min {mn[2] * 1e3:9.1f})  "
                    f"matmul/block-min {med[0] / mn[1]:6.3f} spread {med[1] / mn[1]:5.3f} matmul/torch {med[0] / med[2]:6.2f}  "
                    f"contract bits equal: {same}  max rel diff to torch {err:.2e}")
            del dps, dls, pqs, dp, dl, pq, db
        del pm, w
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
