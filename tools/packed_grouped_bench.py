"""The grouped packed linear (mtq_packed_linear_skinny_grouped) against the routes that exist without it, timed with device events after a
warm-up (the method of DESIGN.md §A.6g: sides alternated in one process, --rounds rounds of a window each, medians and minima).

  grouped : the grouped C entry with a workspace allocated once, one side per value of --splits (0 = the library's choice);
  loop    : mtq_packed_linear_skinny per non-empty group (per 32-row chunk of a larger group) at the library's split, the C entry with
            prebuilt arguments and one workspace: the route a caller has without the grouped entry;
  matmul  : torch.matmul per non-empty group on the unpacked bf16 Ŵ, for information;
  chunked : with --chunked, mtq_packed_linear_skinny_grouped_chunked (a wave per 32-row chunk, the chunk list made on the device) at the
            same splits, alternated with the other sides; its output is compared with the grouped entry's bit for bit, and the run ends
            with the two questions DESIGN.md §A.6m asks of it, answered from this run's numbers alone.

Experts of --shapes (n x k), bf16 storage, maps drawn with 85 % bfp8 and 15 % bfp4 tiles (the mix the greedy search leaves on such
weights), --counts experts.  Routings: `uniform` gives every expert 4 rows; `sparse` spreads 512 rows over the experts with a seeded skewed
draw that leaves many of them empty (the seed and the histogram are printed).

  python tools/packed_grouped_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_linear_grouped.txt] [--json out.json]
  python tools/packed_grouped_bench.py --chunked --out profiles/packed_linear_grouped_chunked.txt
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


def window_ms(fn, iters: int) -> float:
    """Milliseconds per call of `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def calibrate(fn, target_ms: float) -> int:
    fn()
    torch.cuda.synchronize()
    one = max(window_ms(fn, 2), 1e-3)
    return int(min(max(target_ms / one, 3), 200))


def routing(kind: str, count: int, seed: int, rows: int = 512) -> np.ndarray:
    """Rows per expert; `rows`: what the skewed draw spreads (tools/packed_grouped_wide_bench.py spreads a prefill batch with it)."""
    if kind == "uniform":
        return np.full(count, 4, dtype=np.int64)
    rng = np.random.default_rng(seed)
    p = rng.pareto(0.6, size=count) + 1e-3                   # a few hot experts, most cold
    return np.bincount(rng.choice(count, size=rows, p=p / p.sum()), minlength=count).astype(np.int64)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--shapes", default="2048x7168,7168x2048")
    p.add_argument("--counts", default="64,256")
    p.add_argument("--routings", default="uniform,sparse")
    p.add_argument("--splits", default="1,2,4,0")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--chunked", action="store_true", help="add the chunked grouped entry as a side at every split")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# grouped packed linear on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"sides alternated; bf16 output; maps 85% bfp8 / 15% bfp4; seed {args.seed}")
    gentry, sentry = hb._entry("mtq_packed_linear_skinny_grouped"), hb._entry("mtq_packed_linear_skinny")
    centry = hb._entry("mtq_packed_linear_skinny_grouped_chunked") if args.chunked else None
    verdict = []                                             # per row: what the expectation and the rule for "auto" need
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
                per = routing(kind, count, args.seed)
                gr = np.concatenate([[0], np.cumsum(per)])
                T, active = int(gr[-1]), int((per > 0).sum())
                active_mb = sum(pts[e].nbytes for e in range(count) if per[e]) / 1e6
                hist = np.bincount(np.minimum(per, 33), minlength=34)
                say(f"## {n}x{k} count={count} routing={kind}: T={T}, {active} experts with rows ({active_mb:.0f} MB of {stream_mb:.0f} MB of streams), "
                    f"rows per expert max {int(per.max())}; histogram rows:experts "
                    + " ".join(f"{r if r < 33 else '33+'}:{int(c)}" for r, c in enumerate(hist) if c))
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
                grd = torch.from_numpy(gr.astype(np.int32)).cuda()
                ya = torch.zeros((T, n), dtype=torch.bfloat16, device="cuda")
                yb, yc, yd = torch.zeros_like(ya), torch.zeros_like(ya), torch.zeros_like(ya)
                sides = []
                for split in (int(v) for v in args.splits.split(",")):
                    need = hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, split)
                    eff = max(1, need // (4 * T * n))
                    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
                    hb.packed_linear_skinny_grouped(x, grd, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n,
                                                    out_dtype=torch.bfloat16, out=ya, split=split, workspace=ws)   # the wrapper's checks, once
                    call = (x.data_ptr(), T, k, k, grd.data_ptr(), batch.arena.data_ptr(), batch.arena.numel(), batch.maps_dev.data_ptr(),
                            batch.offsets_dev.data_ptr(), batch.bases_dev.data_ptr(), count, n, None, 0, ya.data_ptr(), hb.DTYPE_BF16, n, split,
                            ws.data_ptr(), need, stream)
                    sides.append({"name": f"grouped split={split} (eff {eff})", "split": split, "eff": eff, "ws": ws,
                                  "fn": (lambda call=call: hb.check(gentry(*call)))})
                for split in (int(v) for v in args.splits.split(",")) if args.chunked else ():
                    need = hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, split)
                    eff = max(1, hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, split) // (4 * T * n))
                    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
                    hb.packed_linear_skinny_grouped_chunked(x, grd, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n,
                                                            out_dtype=torch.bfloat16, out=yd, split=split, workspace=ws)   # the wrapper's checks, once
                    hb.packed_linear_skinny_grouped(x, grd, batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, count, n,
                                                    out_dtype=torch.bfloat16, out=ya, split=split)
                    same = bool(torch.equal(yd.view(torch.int16), ya.view(torch.int16)))
                    call = (x.data_ptr(), T, k, k, grd.data_ptr(), batch.arena.data_ptr(), batch.arena.numel(), batch.maps_dev.data_ptr(),
                            batch.offsets_dev.data_ptr(), batch.bases_dev.data_ptr(), count, n, None, 0, yd.data_ptr(), hb.DTYPE_BF16, n, split,
                            ws.data_ptr(), need, stream)
                    sides.append({"name": f"chunked split={split} (eff {eff})", "csplit": split, "eff": eff, "ws": ws, "same": same,
                                  "fn": (lambda call=call: hb.check(centry(*call)))})
                # the loop of single-tensor skinny calls at the library's split, one workspace for all
                chunks = [(e, r, min(32, int(gr[e + 1]) - r)) for e in range(count) for r in range(int(gr[e]), int(gr[e + 1]), 32)]
                need1 = max(hb.packed_linear_skinny_workspace_bytes(c, n, k, 0) for _e, _r, c in chunks)
                ws1 = torch.empty((max(need1, 16),), dtype=torch.uint8, device="cuda")
                lcalls = []
                for e, r, c in chunks:
                    t = pts[e].tables()
                    lcalls.append((x[r:r + c].data_ptr(), c, k, k, pts[e].data.data_ptr(), t.nbytes, t.map_ptr, t.offsets_ptr, n, None, yb[r:r + c].data_ptr(),
                                   hb.DTYPE_BF16, n, 0, ws1.data_ptr(), need1, stream))

                def f_loop():
                    for call in lcalls:
                        hb.check(sentry(*call))

                groups = [(e, int(gr[e]), int(gr[e + 1])) for e in range(count) if per[e]]

                def f_matmul():
                    for e, r0, r1 in groups:
                        torch.matmul(x[r0:r1], what[e].t(), out=yc[r0:r1])

                sides.append({"name": f"loop of {len(lcalls)} skinny calls", "fn": f_loop})
                sides.append({"name": f"loop of {len(groups)} matmuls", "fn": f_matmul})
                for s in sides:
                    s["iters"], s["ts"] = calibrate(s["fn"], args.window_ms), []
                for _ in range(args.rounds):
                    for s in sides:
                        s["ts"].append(window_ms(s["fn"], s["iters"]))
                torch.cuda.synchronize()
                scale = float(yc.float().abs().max().clamp_min(1e-30))
                err_b = float((yb.float() - yc.float()).abs().max()) / scale
                loop_min = min(sides[-2]["ts"])
                if args.chunked:
                    walk = {s["split"]: s["ts"] for s in sides if "split" in s}
                    chunk = {s["csplit"]: s["ts"] for s in sides if "csplit" in s}
                    verdict.append({"row": f"{n}x{k} count={count} {kind}", "kind": kind, "loop_min": loop_min,
                                    "chunk1_median": statistics.median(chunk[1]) if 1 in chunk else None,
                                    "chunk0_median": statistics.median(chunk[0]) if 0 in chunk else None,
                                    "walk0_min": min(walk[0]) if 0 in walk else None,
                                    "spread": max(statistics.median(s["ts"]) / min(s["ts"]) for s in sides[:-1]),   # the packed sides; not torch.matmul's
                                    "same_bits": all(s["same"] for s in sides if "csplit" in s)})
                for s in sides:
                    med, mn = statistics.median(s["ts"]), min(s["ts"])
                    row = {"n": n, "k": k, "count": count, "routing": kind, "T": T, "active": active, "side": s["name"], "ms_median": med,
                           "ms_min": mn, "active_stream_gbs": active_mb / med, "over_loop_min": med / loop_min}
                    extra = ""
                    if "split" in s:
                        s["fn"]()
                        torch.cuda.synchronize()
                        row.update(split=s["split"], split_eff=s["eff"], max_rel_diff=float((ya.float() - yc.float()).abs().max()) / scale)
                        extra = f"  max rel diff to matmul {row['max_rel_diff']:.2e}"
                    if "csplit" in s:
                        row.update(chunked_split=s["csplit"], split_eff=s["eff"], same_bits_as_grouped=s["same"])
                        extra = f"  bits {'equal to' if s['same'] else 'DIFFER from'} grouped at this split"
                    rows_out.append(row)
                    say(f"{s['name']:34s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  {active_mb / med:8.1f} GB/s of "
                        f"active streams  /loop-min {med / loop_min:6.3f}{extra}")
                say(f"{'loop vs matmul':34s} max rel diff {err_b:.2e}")
                del sides, lcalls, x, ya, yb, yc, yd, ws1
            del pts, batch, what
            torch.cuda.empty_cache()
    if verdict and all(v["chunk1_median"] is not None and v["chunk0_median"] is not None and v["walk0_min"] is not None for v in verdict):
        spread = max(v["spread"] for v in verdict)           # the run's own noise: the largest median / min over the packed sides of every row
        say(f"## the questions of DESIGN.md A.6m, from this run alone (spread = largest median/min of any grouped, chunked or loop side of any row = {spread:.4f})")
        say(f"bits: chunked equal to grouped at every row and split: {all(v['same_bits'] for v in verdict)}")
        holds = []
        for v in verdict:
            ok = v["chunk1_median"] < v["loop_min"]
            holds.append(ok)
            say(f"expectation  {v['row']:34s} chunked split=1 median {v['chunk1_median'] * 1e3:9.1f} us {'<' if ok else '>='} loop min "
                f"{v['loop_min'] * 1e3:9.1f} us  ratio {v['chunk1_median'] / v['loop_min']:6.3f}  {'holds' if ok else 'FAILS'}")
        say(f"expectation (chunked split=1 median below the loop's minimum at every row): {'HOLDS' if all(holds) else 'FAILS'} "
            f"({sum(holds)} of {len(holds)} rows)")
        rule = []
        for v in verdict:
            bound = v["walk0_min"] * (1.0 if v["kind"] == "sparse" else spread)
            ok = v["chunk0_median"] < bound if v["kind"] == "sparse" else v["chunk0_median"] <= bound
            rule.append(ok)
            say(f"auto rule    {v['row']:34s} chunked split=0 median {v['chunk0_median'] * 1e3:9.1f} us vs grouped split=0 min "
                f"{v['walk0_min'] * 1e3:9.1f} us{'' if v['kind'] == 'sparse' else f' x spread = {bound * 1e3:9.1f} us'}  ratio "
                f"{v['chunk0_median'] / v['walk0_min']:6.3f}  {'passes' if ok else 'DECIDES AGAINST'}")
        say(f"auto rule (sparse rows: below grouped's min; other rows: within the spread of it): GROUPED_AUTO_KERNEL = "
            f"{'chunks' if all(rule) else 'walk'}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
