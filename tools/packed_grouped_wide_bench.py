"""The grouped wide packed linear (mtq_packed_linear_wide_grouped) at prefill routings against the routes that exist without it, by the
method of tools/packed_grouped_bench.py (device events after a warm-up, sides alternated in one process, --rounds rounds
of a window each, medians and minima), whose helpers, shapes, counts, maps and seeded Pareto draw it uses.

  wide-grouped : the new C entry with its plan workspace allocated once;
  chunked      : mtq_packed_linear_skinny_grouped_chunked at split 0, the best single launch there was;
  wide loop    : mtq_packed_linear_wide per non-empty group, the C entry with prebuilt arguments: the documented route for large groups;
  matmul       : torch.matmul per non-empty group on the unpacked bf16 Ŵ, for information.

Routings: `even128` gives every expert 128 rows, `even64` 64 rows (every 128-row block half empty: the honest bad case), `skew` spreads
64 * count rows by the seeded Pareto draw.  Before any timing the new entry's bf16 output is compared with the wide loop's bit for bit.
The run ends with the expectation DESIGN.md §A.6n set beforehand: the new entry's median below the wide loop's minimum at every row.

  python tools/packed_grouped_wide_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_linear_grouped_wide.txt] [--json out.json]
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
from quantization_analysis_amd import packed
from tools.packed_grouped_bench import calibrate, routing, window_ms


def prefill_routing(kind: str, count: int, seed: int) -> np.ndarray:
    """Rows per expert."""
    if kind == "even128":
        return np.full(count, 128, dtype=np.int64)
    if kind == "even64":
        return np.full(count, 64, dtype=np.int64)
    if kind == "skew":
        return routing("sparse", count, seed, rows=64 * count)
    raise SystemExit(f"unknown routing {kind!r}")


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--shapes", default="2048x7168,7168x2048")
    p.add_argument("--counts", default="64,256")
    p.add_argument("--routings", default="even128,even64,skew")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines, verdict = [], [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# grouped wide packed linear on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"sides alternated; bf16 output; maps 85% bfp8 / 15% bfp4; seed {args.seed}")
    nentry, centry, wentry = (hb._entry(name) for name in ("mtq_packed_linear_wide_grouped", "mtq_packed_linear_skinny_grouped_chunked",
                                                           "mtq_packed_linear_wide"))
    for shape in args.shapes.split(","):
        n, k = (int(v) for v in shape.split("x"))
        th, tw = hb.tiles_hw(n, k)
        for count in (int(v) for v in args.counts.split(",")):
            g = torch.Generator(device="cuda").manual_seed(args.seed + n + count)
            w = torch.empty((count, n, k), dtype=torch.bfloat16, device="cuda")
            for e in range(count):
                w[e] = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            maps = np.random.default_rng(args.seed + count).choice(np.array([1, 2], dtype=np.int8), size=(count, th, tw), p=[0.85, 0.15])
            pts = packed.pack_batch(w, maps, backend="hip")
            batch = packed.batch_of(pts)
            what = packed.unpack_batch(pts, backend="hip", dtype="bfloat16")
            del w
            stream_mb = batch.arena.numel() / 1e6
            for kind in args.routings.split(","):
                per = prefill_routing(kind, count, args.seed)
                gr = np.concatenate([[0], np.cumsum(per)])
                T, active = int(gr[-1]), int((per > 0).sum())
                active_mb = sum(pts[e].nbytes for e in range(count) if per[e]) / 1e6
                blocks, slots = int(sum(-(-int(r) // 128) for r in per)), (T + 127 * min(count, T)) // 128
                say(f"## {n}x{k} count={count} routing={kind}: T={T}, {active} experts with rows ({active_mb:.0f} MB of {stream_mb:.0f} MB of streams), "
                    f"rows per expert min {int(per.min())} median {int(np.median(per))} max {int(per.max())}; {blocks} row blocks in {slots} slots, "
                    f"{int(sum(-(-int(r) // 32) for r in per))} 32-row chunks")
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
                grd = torch.from_numpy(gr.astype(np.int32)).cuda()
                ya = torch.zeros((T, n), dtype=torch.bfloat16, device="cuda")
                yb, yc, yd = torch.zeros_like(ya), torch.zeros_like(ya), torch.zeros_like(ya)
                tables = (batch.arena.data_ptr(), batch.arena.numel(), batch.maps_dev.data_ptr(), batch.offsets_dev.data_ptr(), batch.bases_dev.data_ptr())
                need = hb.packed_linear_wide_grouped_workspace_bytes(T, count, n, k)
                ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
                hb.packed_linear_wide_grouped(x, grd, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n,
                                              out_dtype=torch.bfloat16, out=ya, workspace=ws)             # the wrapper's checks, once
                ncall = (x.data_ptr(), T, k, k, grd.data_ptr(), *tables, count, n, None, 0, ya.data_ptr(), hb.DTYPE_BF16, n, ws.data_ptr(), need, stream)
                cneed = hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, 0)
                ceff = max(1, hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, 0) // (4 * T * n))
                cws = torch.empty((cneed,), dtype=torch.uint8, device="cuda")
                hb.packed_linear_skinny_grouped_chunked(x, grd, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n,
                                                        out_dtype=torch.bfloat16, out=yd, split=0, workspace=cws)
                ccall = (x.data_ptr(), T, k, k, grd.data_ptr(), *tables, count, n, None, 0, yd.data_ptr(), hb.DTYPE_BF16, n, 0, cws.data_ptr(), cneed, stream)
                groups = [(e, int(gr[e]), int(gr[e + 1])) for e in range(count) if per[e]]
                wcalls = []
                for e, r0, r1 in groups:
                    t = pts[e].tables()
                    wcalls.append((x[r0:r1].data_ptr(), r1 - r0, k, k, pts[e].data.data_ptr(), t.nbytes, t.map_ptr, t.offsets_ptr, n, None,
                                   yb[r0:r1].data_ptr(), hb.DTYPE_BF16, n, stream))

                def f_wide_loop():
                    for call in wcalls:
                        hb.check(wentry(*call))

                def f_matmul():
                    for e, r0, r1 in groups:
                        torch.matmul(x[r0:r1], what[e].t(), out=yc[r0:r1])

                f_wide_loop()
                f_matmul()
                torch.cuda.synchronize()
                same = bool(torch.equal(ya.view(torch.int16), yb.view(torch.int16)))                      # before any timing
                scale = float(yc.float().abs().max().clamp_min(1e-30))
                diffs = {name: float((y.float() - yc.float()).abs().max()) / scale for name, y in (("wide-grouped", ya), ("chunked", yd))}
                say(f"{'bits':34s} wide-grouped {'equal to' if same else 'DIFFER from'} the wide loop's; max rel diff to matmul: wide-grouped "
                    f"{diffs['wide-grouped']:.2e}, chunked {diffs['chunked']:.2e}")
                sides = [{"name": "wide-grouped", "fn": (lambda: hb.check(nentry(*ncall)))},
                         {"name": f"chunked split=0 (eff {ceff})", "fn": (lambda: hb.check(centry(*ccall)))},
                         {"name": f"loop of {len(wcalls)} wide calls", "fn": f_wide_loop},
                         {"name": f"loop of {len(groups)} matmuls", "fn": f_matmul}]
                for s in sides:
                    s["iters"], s["ts"] = calibrate(s["fn"], args.window_ms), []
                for _ in range(args.rounds):
                    for s in sides:
                        s["ts"].append(window_ms(s["fn"], s["iters"]))
                torch.cuda.synchronize()
                loop_min = min(sides[2]["ts"])
                verdict.append({"row": f"{n}x{k} count={count} {kind}", "new_median": statistics.median(sides[0]["ts"]), "loop_min": loop_min,
                                "chunked_median": statistics.median(sides[1]["ts"]), "same_bits": same})
                for s in sides:
                    med, mn = statistics.median(s["ts"]), min(s["ts"])
                    rows_out.append({"n": n, "k": k, "count": count, "routing": kind, "T": T, "active": active, "side": s["name"], "ms_median": med,
                                     "ms_min": mn, "active_stream_gbs": active_mb / med, "over_wide_loop_min": med / loop_min,
                                     "tflops": 2.0 * T * n * k / med / 1e9, "same_bits_as_wide_loop": same})
                    say(f"{s['name']:34s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  "
                        f"{2.0 * T * n * k / med / 1e9:7.1f} TFLOP/s  /wide-loop-min {med / loop_min:6.3f}")
                del sides, wcalls, x, ya, yb, yc, yd, ws, cws
            del pts, batch, what
            torch.cuda.empty_cache()
    say("## the expectation of DESIGN.md A.6n, from this run alone")
    say(f"bits: wide-grouped equal to the wide loop at every row: {all(v['same_bits'] for v in verdict)}")
    holds = []
    for v in verdict:
        ok = v["new_median"] < v["loop_min"]
        holds.append(ok)
        say(f"expectation  {v['row']:34s} wide-grouped median {v['new_median'] * 1e3:9.1f} us {'<' if ok else '>='} wide loop min "
            f"{v['loop_min'] * 1e3:9.1f} us  ratio {v['new_median'] / v['loop_min']:6.3f}  {'holds' if ok else 'FAILS'}   "
            f"(chunked split=0 median {v['chunked_median'] * 1e3:9.1f} us, x{v['chunked_median'] / v['new_median']:5.2f} of wide-grouped)")
    say(f"expectation (wide-grouped median below the wide loop's minimum at every row): {'HOLDS' if all(holds) else 'FAILS'} "
        f"({sum(holds)} of {len(holds)} rows)")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
