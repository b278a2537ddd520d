"""The packed mixed-tile kernels (csrc/mtq_packed.hip), timed with device events after a warm-up.

  pack / unpack : one n × k bf16 weight under an all-bfp8, an all-bfp4 and a greedy map; bytes moved (input + stream, stream + output)
                  over time, against the HBM figure (--hbm-tbs, 8 TB/s).
  packed_linear : n × k in {4096², 14336 × 4096}, m in {1, 16, 256, 4096}, the same three maps, alternated in the same process with
                  torch.matmul on the unpacked bf16 Ŵ (hipBLASLt), --rounds rounds of a window each; median and minimum per call.
                  The weight stream is what bounds small m, so both sides rotate over enough copies of the weight (--cold-mb in all)
                  that a call does not find the previous call's weight in the 256 MiB Infinity Cache.  GB/s = the packed stream's
                  bytes over the packed kernel's time; for matmul, the bf16 weight's bytes over its time.
  skinny        : for m <= 32 the split-K kernel (mtq_packed_linear_skinny, the C entry with a preallocated workspace) is a third side
                  of the same alternation, once per value of --splits (0 = the library's choice); `skinny/block-min` is the skinny
                  median over the block kernel's MINIMUM of the same run, the gate of DESIGN.md §A.6h.

  wide          : --wide adds the wide-block kernel for m above the decode range (mtq_packed_linear_wide, the C entry) as one more
                  side of the same alternation; `wide/block-min` is the wide median over the block kernel's MINIMUM of the same run,
                  the gate of DESIGN.md §A.6k; the line also says whether the result's bits are the block kernel's.

  python tools/packed_linear_bench.py [--rounds 5] [--window-ms 30] [--out profiles/packed_linear.txt] [--json out.json]
  python tools/packed_linear_bench.py --linear-only --ms 1,4,16,32 --out profiles/packed_linear_skinny.txt
  python tools/packed_linear_bench.py --linear-only --wide --ms 64,128,256,512,1024,2048,4096 --out profiles/packed_linear_wide.txt
  (the record kept there also has rows=256 lines: a 256 x 128 instantiation that was measured beside the kernel, lost and was removed)
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

FMTS = ["bf16", "bfp8", "bfp4", "bfp2"]


def window_ms(fn, iters: int) -> float:
    """Milliseconds per call of `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def calibrate(fn, target_ms: float) -> int:
    fn(0)
    torch.cuda.synchronize()
    one = max(window_ms(fn, 3), 1e-3)
    return int(min(max(target_ms / one, 5), 400))


def greedy_map(w) -> np.ndarray:
    """The greedy search's map of a bf16 weight (pcc 0.999, seed 123), on the device."""
    recs = hb.tile_stats_batched(w[None], 0xE)
    seeds = torch.tensor([123], dtype=torch.int64, device="cuda")
    maps, status = hb.greedy_scan_device(recs, 0xE | hb.MASK_BF16_IDENTITY, FMTS, "pcc", 0.999, float(w.numel()), seeds)
    assert int(status.cpu()[0]) == 0
    return maps.cpu().numpy().reshape(hb.tiles_hw(*w.shape)).astype(np.int8)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=30.0)
    p.add_argument("--cold-mb", type=float, default=640.0, help="rotate over copies of the weight worth this many MB")
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--shapes", default="4096x4096,14336x4096")
    p.add_argument("--ms", default="1,16,256,4096")
    p.add_argument("--splits", default="0", help="skinny side: the split values to time, comma separated (0: the library's choice)")
    p.add_argument("--wide", action="store_true", help="time the wide-block kernel beside the block kernel and torch.matmul")
    p.add_argument("--linear-only", action="store_true", help="skip the pack / unpack timings")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    rows, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# packed kernels on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"weights rotated over {args.cold_mb:.0f} MB; HBM figure {args.hbm_tbs} TB/s")
    for shape in args.shapes.split(","):
        n, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + k)
        w = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        th, tw = hb.tiles_hw(n, k)
        maps = {"bfp8": np.full((th, tw), 1, dtype=np.int8), "bfp4": np.full((th, tw), 2, dtype=np.int8), "greedy": greedy_map(w)}
        for name, amap in maps.items():
            tables = hb.PackedTables.on_device(amap)
            data = hb.pack_tiles(w, tables)
            counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
            wq = hb.unpack_tiles(data, tables, n, k, dtype=torch.bfloat16)
            y32 = torch.empty((n, k), dtype=torch.float32, device="cuda")
            # pack / unpack: bytes moved over time
            for what, fn, moved in () if args.linear_only else (("pack", lambda i: hb.pack_tiles(w, tables, out=data), 2 * n * k + tables.nbytes),
                                    ("unpack_bf16", lambda i: hb.unpack_tiles(data, tables, n, k, dtype=torch.bfloat16, out=wq), tables.nbytes + 2 * n * k),
                                    ("unpack_f32", lambda i: hb.unpack_tiles(data, tables, n, k, out=y32), tables.nbytes + 4 * n * k)):
                iters = calibrate(fn, args.window_ms)
                ts = [window_ms(fn, iters) for _ in range(args.rounds)]
                med = statistics.median(ts)
                rows.append({"what": what, "n": n, "k": k, "map": name, "counts": counts, "ms_median": med, "ms_min": min(ts), "bytes": moved,
                             "gbs": moved / med / 1e6, "hbm_fraction": moved / med / 1e6 / (args.hbm_tbs * 1e3)})
                say(f"{what:12s} {n}x{k} map={name:6s} counts={counts} {med * 1e3:9.1f} us (min {min(ts) * 1e3:9.1f})  {moved / med / 1e6:8.1f} GB/s "
                    f"= {100 * moved / med / 1e6 / (args.hbm_tbs * 1e3):5.1f}% of {args.hbm_tbs} TB/s")
            del y32
            # linear against torch.matmul on the unpacked bf16 weight, alternated
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / tables.nbytes)))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (2 * n * k))))
            datas = [data] + [data.clone() for _ in range(copies_p - 1)]
            wqs = [wq] + [wq.clone() for _ in range(copies_w - 1)]
            for m in (int(v) for v in args.ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                yp = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
                ym = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")

                hb.packed_linear(x, data, tables, n, out_dtype=torch.bfloat16, out=yp)   # the wrapper's checks, once
                entry, stream = hb._entry("mtq_packed_linear"), torch.cuda.current_stream().cuda_stream
                calls = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tables.nbytes, tables.map_ptr, tables.offsets_ptr, n, None, yp.data_ptr(),
                          hb.DTYPE_BF16, n, stream) for d in datas]

                def f_packed(i):   # the C entry itself: at m = 1 the binding's Python checks would be what is timed
                    hb.check(entry(*calls[i % copies_p]))

                def f_matmul(i):
                    torch.matmul(x, wqs[i % copies_w].t(), out=ym)

                # the skinny kernel, one side per split: the C entry with a workspace allocated once
                skinny = []
                if m <= hb.PACKED_SKINNY_MAX_M:
                    ys = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
                    sentry = hb._entry("mtq_packed_linear_skinny")
                    for split in (int(v) for v in args.splits.split(",")):
                        need = hb.packed_linear_skinny_workspace_bytes(m, n, k, split)
                        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
                        hb.packed_linear_skinny(x, data, tables, n, out_dtype=torch.bfloat16, out=ys, split=split, workspace=ws)   # the checks, once
                        scalls = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tables.nbytes, tables.map_ptr, tables.offsets_ptr, n, None,
                                   ys.data_ptr(), hb.DTYPE_BF16, n, split, ws.data_ptr(), need, stream) for d in datas]

                        def f_skinny(i, scalls=scalls):
                            hb.check(sentry(*scalls[i % copies_p]))

                        skinny.append({"split": split, "workspace_bytes": need, "fn": f_skinny, "ws": ws, "iters": calibrate(f_skinny, args.window_ms),
                                       "ts": []})

                # the wide kernel: the C entry, as the block side
                wide = []
                if args.wide:
                    yw = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
                    hb.packed_linear_wide(x, data, tables, n, out_dtype=torch.bfloat16, out=yw)   # the wrapper's checks, once
                    wentry = hb._entry("mtq_packed_linear_wide")
                    wcalls = [c[:10] + (yw.data_ptr(),) + c[11:] for c in calls]

                    def f_wide(i):
                        hb.check(wentry(*wcalls[i % copies_p]))

                    wide.append({"fn": f_wide, "iters": calibrate(f_wide, args.window_ms), "ts": []})

                ip, im = calibrate(f_packed, args.window_ms), calibrate(f_matmul, args.window_ms)
                tp, tm = [], []
                for _ in range(args.rounds):
                    tp.append(window_ms(f_packed, ip))
                    for side in wide:
                        side["ts"].append(window_ms(side["fn"], side["iters"]))
                    for side in skinny:
                        side["ts"].append(window_ms(side["fn"], side["iters"]))
                    tm.append(window_ms(f_matmul, im))
                f_packed(0)
                f_matmul(0)
                err = float((yp.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                mp, mm = statistics.median(tp), statistics.median(tm)
                rows.append({"what": "packed_linear", "n": n, "k": k, "m": m, "map": name, "counts": counts, "packed_ms_median": mp,
                             "packed_ms_min": min(tp), "matmul_ms_median": mm, "matmul_ms_min": min(tm), "packed_over_matmul": mp / mm,
                             "packed_stream_gbs": tables.nbytes / mp / 1e6, "matmul_weight_gbs": 2 * n * k / mm / 1e6,
                             "packed_tflops": 2.0 * m * n * k / mp / 1e9, "matmul_tflops": 2.0 * m * n * k / mm / 1e9, "max_rel_diff": err})
                say(f"linear       {n}x{k} m={m:5d} map={name:6s} packed {mp * 1e3:9.1f} us (min {min(tp) * 1e3:9.1f}, {tables.nbytes / mp / 1e6:7.1f} GB/s of stream) "
                    f"matmul {mm * 1e3:9.1f} us (min {min(tm) * 1e3:9.1f}, {2 * n * k / mm / 1e6:7.1f} GB/s of bf16 W)  packed/matmul {mp / mm:6.2f}  "
                    f"max rel diff {err:.2e}")
                flop = 2.0 * m * n * k
                for side in wide:
                    yw.zero_()
                    side["fn"](0)
                    same = bool(torch.equal(yw.view(torch.int16), yp.view(torch.int16)))
                    mw, mnw = statistics.median(side["ts"]), min(side["ts"])
                    rows.append({"what": "packed_linear_wide", "n": n, "k": k, "m": m, "map": name, "counts": counts,
                                 "wide_ms_median": mw, "wide_ms_min": mnw, "block_ms_median": mp, "block_ms_min": min(tp), "matmul_ms_median": mm,
                                 "matmul_ms_min": min(tm), "wide_over_block_min": mw / min(tp), "wide_over_matmul": mw / mm,
                                 "wide_tflops": flop / mw / 1e9, "block_tflops": flop / mp / 1e9, "matmul_tflops": flop / mm / 1e9,
                                 "bits_equal_block": same})
                    say(f"wide         {n}x{k} m={m:5d} map={name:6s} {mw * 1e3:9.1f} us (min {mnw * 1e3:9.1f}, "
                        f"{flop / mw / 1e9:7.1f} TFLOP/s; block {flop / mp / 1e9:7.1f}, matmul {flop / mm / 1e9:7.1f})  wide/block-min {mw / min(tp):6.3f}  "
                        f"wide/matmul {mw / mm:6.2f}  bits equal block: {same}")
                del wide
                for side in skinny:
                    side["fn"](0)
                    serr = float((ys.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                    ms_, mn_ = statistics.median(side["ts"]), min(side["ts"])
                    rows.append({"what": "packed_linear_skinny", "n": n, "k": k, "m": m, "map": name, "counts": counts, "split": side["split"],
                                 "workspace_bytes": side["workspace_bytes"], "skinny_ms_median": ms_, "skinny_ms_min": mn_,
                                 "block_ms_median": mp, "block_ms_min": min(tp), "matmul_ms_median": mm, "skinny_over_block_min": ms_ / min(tp),
                                 "skinny_over_matmul": ms_ / mm, "skinny_stream_gbs": tables.nbytes / ms_ / 1e6, "max_rel_diff": serr})
                    say(f"skinny       {n}x{k} m={m:5d} map={name:6s} split={side['split']:3d} {ms_ * 1e3:9.1f} us (min {mn_ * 1e3:9.1f}, "
                        f"{tables.nbytes / ms_ / 1e6:7.1f} GB/s of stream)  skinny/block-min {ms_ / min(tp):6.3f}  skinny/matmul {ms_ / mm:6.2f}  "
                        f"max rel diff {serr:.2e}")
                del skinny
            del datas, wqs, data, wq
        del w
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
