"""The gated product on packed weights (mtq_packed_glu_wide, mtq_packed_glu_wide_grouped) against the routes that exist without the
fused kernel, by the method of DESIGN.md §A.6g: device events after a warm-up, the sides alternated in one process, --rounds rounds of a
window each, medians and minima, the C entries called directly with prebuilt arguments, bf16 output, and both sides rotating over enough
copies of the weights (--cold-mb in all) that a call does not find the previous call's weights in the 256 MiB Infinity Cache.

  fused    : mtq_packed_glu_wide, one launch;
  unfused  : two mtq_packed_linear_wide calls into float32 and mtq_glu_combine: the same bits as fused (checked before any timing);
  today    : what a user had before: two mtq_packed_linear_wide calls into bf16 and torch's silu(g) * u;
  matmul   : torch.matmul twice on the unpacked bf16 weights and torch's silu(g) * u, for information.

Dense rows: n x k in --shapes, m in --ms, maps all-bfp8, all-bfp4 and the 85 / 15 mix of the two.  Grouped rows (--grouped-shapes,
--counts): tools/packed_grouped_wide_bench.py's `even128` and `skew` routings, with mtq_packed_linear_wide_grouped in place of the wide
entry on the unfused and today sides.  The run ends with the rule of packed.AUTO_GLU_FUSED_MIN_M applied to its own dense rows: the
smallest m from which on the fused median is below the unfused minimum at every shape and map, or None.

  python tools/packed_glu_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_glu.txt] [--json out.json]

--decode times the decode range instead, by the same method:

  fused    : mtq_packed_glu_skinny at split 0, two launches;
  pair     : the baseline, what glu(kernel="auto") runs at m <= 32: two mtq_packed_linear_skinny calls into float32 and mtq_glu_combine,
             five launches, the same bits as fused (checked before any timing);
  matmul   : torch.matmul twice on the unpacked bf16 weights and torch's silu(g) * u, for information.

Dense rows: n x k in --shapes, m in --decode-ms, maps all-bfp8, all-bfp4 and the mix.  Grouped rows: --decode-grouped-shape with --counts
experts under the routings `one` (a row per expert), `eight32` (8 rows in each of 32 experts) and `skew`: mtq_packed_glu_skinny_grouped
against two mtq_packed_linear_skinny_grouped calls and the combine (the baseline) and mtq_packed_glu_wide_grouped.  Then the new entry at
explicit splits (--sweep) on the first shape under bfp8, and the gate: at every row the fused median must be below the baseline's minimum
by more than the baseline's own minimum-to-median spread.

  python tools/packed_glu_bench.py --decode [--out profiles/packed_glu_skinny.txt]
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
from tools.packed_grouped_bench import routing as grouped_routing
from tools.packed_grouped_wide_bench import prefill_routing
from tools.packed_linear_bench import calibrate, window_ms


def mixed_map(th: int, tw: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).choice(np.array([1, 2], dtype=np.int8), size=(th, tw), p=[0.85, 0.15])


def time_sides(sides, rounds: int, target_ms: float) -> None:
    for s in sides:
        s["iters"], s["ts"] = calibrate(s["fn"], target_ms), []
    for _ in range(rounds):
        for s in sides:
            s["ts"].append(window_ms(s["fn"], s["iters"]))
    torch.cuda.synchronize()


def decode_routing(kind: str, count: int, seed: int) -> np.ndarray:
    """Rows per expert of a decode step."""
    if kind == "one":
        return np.ones(count, dtype=np.int64)
    if kind == "eight32":
        per = np.zeros(count, dtype=np.int64)
        per[np.random.default_rng(seed).choice(count, size=32, replace=False)] = 8
        return per
    return grouped_routing("skew", count, seed, rows=256)


def decode(args) -> int:
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines, gate_rows = [], [], []
    silu, bf16, f32 = hb.ACT_CODE["silu"], hb.DTYPE_BF16, hb.DTYPE_F32

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides, same):
        base = sides[1]
        base_min, base_med = min(base["ts"]), statistics.median(base["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            rows_out.append({**label, "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3, "over_baseline_min": med / base_min,
                             "bits_equal_baseline": same})
            say(f"{s['name']:10s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  /{base['name']}-min {med / base_min:6.3f}")
        fused = statistics.median(sides[0]["ts"])
        gate_rows.append({**label, "fused_median": fused, "base_min": base_min, "base_spread": base_med - base_min, "same": same})

    say(f"# packed SwiGLU for decode on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"sides alternated; bf16 output; weights rotated over {args.cold_mb:.0f} MB; seed {args.seed}")
    fentry, sentry, centry = (hb._entry(name) for name in ("mtq_packed_glu_skinny", "mtq_packed_linear_skinny", "mtq_glu_combine"))
    sweep_done = False
    for shape in (s for s in args.shapes.split(",") if s):
        n, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(args.seed + n + k)
        wg, wu = ((torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(2))
        th, tw = hb.tiles_hw(n, k)
        for name, mg, mu in (("bfp8", np.full((th, tw), 1, dtype=np.int8), np.full((th, tw), 1, dtype=np.int8)),
                             ("bfp4", np.full((th, tw), 2, dtype=np.int8), np.full((th, tw), 2, dtype=np.int8)),
                             ("mix", mixed_map(th, tw, args.seed), mixed_map(th, tw, args.seed + 1))):
            tg, tu = hb.PackedTables.on_device(mg), hb.PackedTables.on_device(mu)
            dg, du = hb.pack_tiles(wg, tg), hb.pack_tiles(wu, tu)
            qg, qu = hb.unpack_tiles(dg, tg, n, k, dtype=torch.bfloat16), hb.unpack_tiles(du, tu, n, k, dtype=torch.bfloat16)
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / (tg.nbytes + tu.nbytes))))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (4 * n * k))))
            dgs, dus = [dg] + [dg.clone() for _ in range(copies_p - 1)], [du] + [du.clone() for _ in range(copies_p - 1)]
            qgs, qus = [qg] + [qg.clone() for _ in range(copies_w - 1)], [qu] + [qu.clone() for _ in range(copies_w - 1)]
            for m in (int(v) for v in args.decode_ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                yf, yp, ym, s16, u16 = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(5))
                g32, u32 = (torch.empty((m, n), dtype=torch.float32, device="cuda") for _ in range(2))

                def workspace(size):
                    return torch.empty((max(size, 16),), dtype=torch.uint8, device="cuda")

                def fused_calls(split):
                    need = hb.packed_glu_skinny_workspace_bytes(m, n, k, split)
                    ws = workspace(need)
                    return ws, [(x.data_ptr(), m, k, k, a.data_ptr(), tg.nbytes, tg.map_ptr, tg.offsets_ptr, b.data_ptr(), tu.nbytes, tu.map_ptr,
                                 tu.offsets_ptr, n, None, None, silu, yf.data_ptr(), bf16, n, split, ws.data_ptr(), need, stream) for a, b in zip(dgs, dus)]

                hb.packed_glu_skinny(x, dg, tg, du, tu, n, out_dtype=torch.bfloat16, out=yf)        # the wrapper's checks, once
                fws, fcalls = fused_calls(0)
                need1 = hb.packed_linear_skinny_workspace_bytes(m, n, k, 0)
                wsg, wsu = workspace(need1), workspace(need1)
                pcalls = [((x.data_ptr(), m, k, k, a.data_ptr(), tg.nbytes, tg.map_ptr, tg.offsets_ptr, n, None, g32.data_ptr(), f32, n, 0,
                            wsg.data_ptr() if need1 else None, need1, stream),
                           (x.data_ptr(), m, k, k, b.data_ptr(), tu.nbytes, tu.map_ptr, tu.offsets_ptr, n, None, u32.data_ptr(), f32, n, 0,
                            wsu.data_ptr() if need1 else None, need1, stream)) for a, b in zip(dgs, dus)]
                ccall = (g32.data_ptr(), n, u32.data_ptr(), n, m, n, silu, yp.data_ptr(), bf16, n, stream)

                def f_fused(i):
                    hb.check(fentry(*fcalls[i % copies_p]))

                def f_pair(i):
                    a, b = pcalls[i % copies_p]
                    hb.check(sentry(*a))
                    hb.check(sentry(*b))
                    hb.check(centry(*ccall))

                def f_matmul(i):
                    torch.matmul(x, qgs[i % copies_w].t(), out=s16)
                    torch.matmul(x, qus[i % copies_w].t(), out=u16)
                    torch.nn.functional.silu(s16, inplace=True)
                    torch.mul(s16, u16, out=ym)

                f_fused(0)
                f_pair(0)
                f_matmul(0)
                torch.cuda.synchronize()
                same = bool(torch.equal(yf.view(torch.int16), yp.view(torch.int16)))            # before any timing
                err = float((yf.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                eff = hb.packed_glu_skinny_workspace_bytes(m, n, k, 0) // (8 * m * n)
                say(f"## {n}x{k} m={m} map={name}: split {eff}; fused bits {'equal to' if same else 'DIFFER from'} the pair's; max rel diff to the "
                    f"matmul side {err:.2e}")
                sides = [{"name": "fused", "fn": f_fused}, {"name": "pair", "fn": f_pair}, {"name": "matmul", "fn": f_matmul}]
                time_sides(sides, args.rounds, args.window_ms)
                report({"what": "glu_skinny", "row": f"{n}x{k} m={m} {name}"}, sides, same)
                if not sweep_done and name == "bfp8":
                    sw = []
                    for split in (int(v) for v in args.sweep.split(",")):
                        ws, calls = fused_calls(split)
                        sw.append({"name": f"split {split}", "ws": ws, "fn": (lambda i, calls=calls: hb.check(fentry(*calls[i % copies_p])))})
                    sw.append({"name": f"split 0={eff}", "fn": f_fused})
                    time_sides(sw, args.rounds, args.window_ms)
                    best = min(statistics.median(s["ts"]) for s in sw)
                    say(f"### the new entry at explicit splits, {n}x{k} m={m} bfp8 ({2 * th} x split units; the rule's own split last)")
                    for s in sw:
                        med, mn = statistics.median(s["ts"]), min(s["ts"])
                        rows_out.append({"what": "sweep", "row": f"{n}x{k} m={m}", "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3})
                        say(f"{s['name']:12s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f})  /best {med / best:6.3f}")
                    del sw
                del sides, fcalls, pcalls
            sweep_done = True
            del dgs, dus, qgs, qus, dg, du, qg, qu
            torch.cuda.empty_cache()
        del wg, wu

    # ---- grouped
    gfentry, gsentry, gwentry = (hb._entry(name) for name in ("mtq_packed_glu_skinny_grouped", "mtq_packed_linear_skinny_grouped",
                                                              "mtq_packed_glu_wide_grouped"))
    n, k = (int(v) for v in args.decode_grouped_shape.split("x"))
    th, tw = hb.tiles_hw(n, k)
    for count in (int(v) for v in args.counts.split(",")):
        g = torch.Generator(device="cuda").manual_seed(args.seed + n + count)
        batches = []
        for side in range(2):
            w = torch.empty((count, n, k), dtype=torch.bfloat16, device="cuda")
            for e in range(count):
                w[e] = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            maps = np.random.default_rng(args.seed + count + side).choice(np.array([1, 2], dtype=np.int8), size=(count, th, tw), p=[0.85, 0.15])
            batches.append(packed.batch_of(packed.pack_batch(w, maps, backend="hip")))
            del w
        gb, ub = batches
        for kind in ("one", "eight32", "skew"):
            per = decode_routing(kind, count, args.seed)
            gr = np.concatenate([[0], np.cumsum(per)])
            T = int(gr[-1])
            x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
            grd = torch.from_numpy(gr.astype(np.int32)).cuda()
            yf, yp, yw = (torch.zeros((T, n), dtype=torch.bfloat16, device="cuda") for _ in range(3))
            g32, u32 = (torch.zeros((T, n), dtype=torch.float32, device="cuda") for _ in range(2))
            need = hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, 0)
            need1 = hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, 0)
            needw = hb.packed_glu_wide_grouped_workspace_bytes(T, count, n, k)
            ws, wsg, wsu, wsw = (torch.empty((max(v, 16),), dtype=torch.uint8, device="cuda") for v in (need, need1, need1, needw))
            tabs = [(b.arena.data_ptr(), b.arena.numel(), b.maps_dev.data_ptr(), b.offsets_dev.data_ptr(), b.bases_dev.data_ptr()) for b in (gb, ub)]
            hb.packed_glu_skinny_grouped(x, grd, (gb.arena, gb.maps_dev, gb.offsets_dev, gb.bases_dev), (ub.arena, ub.maps_dev, ub.offsets_dev, ub.bases_dev),
                                         count, n, out_dtype=torch.bfloat16, out=yf, workspace=ws)       # the wrapper's checks, once
            fcall = (x.data_ptr(), T, k, k, grd.data_ptr(), *tabs[0], *tabs[1], count, n, None, None, 0, silu, yf.data_ptr(), bf16, n, 0, ws.data_ptr(), need, stream)
            wcall = (x.data_ptr(), T, k, k, grd.data_ptr(), *tabs[0], *tabs[1], count, n, None, None, 0, silu, yw.data_ptr(), bf16, n, wsw.data_ptr(), needw, stream)
            pcalls = [(x.data_ptr(), T, k, k, grd.data_ptr(), *tab, count, n, None, 0, out.data_ptr(), f32, n, 0, w_.data_ptr() if need1 else None, need1, stream)
                      for tab, out, w_ in ((tabs[0], g32, wsg), (tabs[1], u32, wsu))]
            ccall = (g32.data_ptr(), n, u32.data_ptr(), n, T, n, silu, yp.data_ptr(), bf16, n, stream)

            def f_fused(i):
                hb.check(gfentry(*fcall))

            def f_pair(i):
                hb.check(gsentry(*pcalls[0]))
                hb.check(gsentry(*pcalls[1]))
                hb.check(centry(*ccall))

            def f_wide(i):
                hb.check(gwentry(*wcall))

            f_fused(0)
            f_pair(0)
            torch.cuda.synchronize()
            same = bool(torch.equal(yf.view(torch.int16), yp.view(torch.int16)))
            say(f"## grouped {n}x{k} count={count} routing={kind}: T={T}, rows per expert min {int(per.min())} median {int(np.median(per))} max "
                f"{int(per.max())}, {(gb.arena.numel() + ub.arena.numel()) / 1e6:.0f} MB of streams, split {need // (8 * T * n)}; fused bits "
                f"{'equal to' if same else 'DIFFER from'} the pair's")
            sides = [{"name": "fused", "fn": f_fused}, {"name": "pair", "fn": f_pair}, {"name": "wide", "fn": f_wide}]
            time_sides(sides, args.rounds, args.window_ms)
            report({"what": "glu_skinny_grouped", "row": f"grouped {n}x{k} count={count} {kind}"}, sides, same)
            del sides, x, yf, yp, yw, g32, u32
        del batches, gb, ub
        torch.cuda.empty_cache()

    say("## the gate: the fused median below the baseline's minimum by more than the baseline's own minimum-to-median spread")
    say(f"bits: fused equal to the baseline at every row: {all(r['same'] for r in gate_rows)}")
    for what in ("glu_skinny", "glu_skinny_grouped"):
        at = [r for r in gate_rows if r["what"] == what]
        if not at:
            continue
        passed = [r for r in at if r["fused_median"] < r["base_min"] - r["base_spread"]]
        ratios = [r["fused_median"] / r["base_min"] for r in at]
        say(f"{what}: {len(passed)} of {len(at)} rows pass; fused median / baseline minimum {min(ratios):6.3f} .. {max(ratios):6.3f}")
        for r in at:
            if r not in passed:
                say(f"  fails at {r['row']}: ratio {r['fused_median'] / r['base_min']:6.3f}, baseline spread {r['base_spread'] / r['base_min'] * 100:4.1f}%")
        say(f"{what}: verdict {'PASS' if len(passed) == len(at) else 'FAIL'}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--cold-mb", type=float, default=640.0, help="rotate over copies of the two weights worth this many MB")
    p.add_argument("--shapes", default="4096x4096,14336x4096")
    p.add_argument("--ms", default="64,128,256,512,1024,4096")
    p.add_argument("--grouped-shapes", default="2048x7168,7168x2048")
    p.add_argument("--counts", default="64,256")
    p.add_argument("--routings", default="even128,skew")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--decode", action="store_true", help="time the decode range: the fused split-K entries against the skinny pair and the combine")
    p.add_argument("--decode-ms", default="1,8,16,32")
    p.add_argument("--decode-grouped-shape", default="2048x7168")
    p.add_argument("--sweep", default="1,2,4,8,16,32,64,128", help="--decode: the explicit splits of the new entry on the first shape under bfp8")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    if args.decode:
        return decode(args)
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines, gate_rows = [], [], []
    silu, bf16, f32 = hb.ACT_CODE["silu"], hb.DTYPE_BF16, hb.DTYPE_F32

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides, flop, same):
        unfused_min = min(sides[1]["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            rows_out.append({**label, "side": s["name"], "ms_median": med, "ms_min": mn, "tflops": flop / med / 1e9,
                             "over_unfused_min": med / unfused_min, "fused_bits_equal_unfused": same})
            say(f"{s['name']:10s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  {flop / med / 1e9:7.1f} TFLOP/s  "
                f"/unfused-min {med / unfused_min:6.3f}")
        return statistics.median(sides[0]["ts"]), unfused_min

    say(f"# packed SwiGLU on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, sides "
        f"alternated; bf16 output; weights rotated over {args.cold_mb:.0f} MB; seed {args.seed}")
    fentry, wentry, centry = (hb._entry(name) for name in ("mtq_packed_glu_wide", "mtq_packed_linear_wide", "mtq_glu_combine"))
    for shape in (s for s in args.shapes.split(",") if s):
        n, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(args.seed + n + k)
        wg, wu = ((torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(2))
        th, tw = hb.tiles_hw(n, k)
        for name, mg, mu in (("bfp8", np.full((th, tw), 1, dtype=np.int8), np.full((th, tw), 1, dtype=np.int8)),
                             ("bfp4", np.full((th, tw), 2, dtype=np.int8), np.full((th, tw), 2, dtype=np.int8)),
                             ("mix", mixed_map(th, tw, args.seed), mixed_map(th, tw, args.seed + 1))):
            tg, tu = hb.PackedTables.on_device(mg), hb.PackedTables.on_device(mu)
            dg, du = hb.pack_tiles(wg, tg), hb.pack_tiles(wu, tu)
            qg, qu = hb.unpack_tiles(dg, tg, n, k, dtype=torch.bfloat16), hb.unpack_tiles(du, tu, n, k, dtype=torch.bfloat16)
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / (tg.nbytes + tu.nbytes))))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (4 * n * k))))
            dgs, dus = [dg] + [dg.clone() for _ in range(copies_p - 1)], [du] + [du.clone() for _ in range(copies_p - 1)]
            qgs, qus = [qg] + [qg.clone() for _ in range(copies_w - 1)], [qu] + [qu.clone() for _ in range(copies_w - 1)]
            for m in (int(v) for v in args.ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                yf, yu, yt, ym = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(4))
                g32, u32 = (torch.empty((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
                g16, u16, s16 = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(3))
                hb.packed_glu_wide(x, dg, tg, du, tu, n, out_dtype=torch.bfloat16, out=yf)          # the wrapper's checks, once
                fcalls = [(x.data_ptr(), m, k, k, a.data_ptr(), tg.nbytes, tg.map_ptr, tg.offsets_ptr, b.data_ptr(), tu.nbytes, tu.map_ptr,
                           tu.offsets_ptr, n, None, None, silu, yf.data_ptr(), bf16, n, stream) for a, b in zip(dgs, dus)]

                def wide_calls(out_g, out_u, code):
                    return [((x.data_ptr(), m, k, k, a.data_ptr(), tg.nbytes, tg.map_ptr, tg.offsets_ptr, n, None, out_g.data_ptr(), code, n, stream),
                             (x.data_ptr(), m, k, k, b.data_ptr(), tu.nbytes, tu.map_ptr, tu.offsets_ptr, n, None, out_u.data_ptr(), code, n, stream))
                            for a, b in zip(dgs, dus)]

                ucalls, tcalls = wide_calls(g32, u32, f32), wide_calls(g16, u16, bf16)
                ccall = (g32.data_ptr(), n, u32.data_ptr(), n, m, n, silu, yu.data_ptr(), bf16, n, stream)

                def f_fused(i):
                    hb.check(fentry(*fcalls[i % copies_p]))

                def f_unfused(i):
                    a, b = ucalls[i % copies_p]
                    hb.check(wentry(*a))
                    hb.check(wentry(*b))
                    hb.check(centry(*ccall))

                def f_today(i):
                    a, b = tcalls[i % copies_p]
                    hb.check(wentry(*a))
                    hb.check(wentry(*b))
                    torch.nn.functional.silu(g16, inplace=True)
                    torch.mul(g16, u16, out=yt)

                def f_matmul(i):
                    torch.matmul(x, qgs[i % copies_w].t(), out=s16)
                    torch.matmul(x, qus[i % copies_w].t(), out=u16)
                    torch.nn.functional.silu(s16, inplace=True)
                    torch.mul(s16, u16, out=ym)

                f_fused(0)
                f_unfused(0)
                f_matmul(0)
                torch.cuda.synchronize()
                same = bool(torch.equal(yf.view(torch.int16), yu.view(torch.int16)))            # before any timing
                err = float((yf.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                say(f"## {n}x{k} m={m} map={name}: fused bits {'equal to' if same else 'DIFFER from'} unfused; max rel diff to the matmul side {err:.2e}")
                sides = [{"name": "fused", "fn": f_fused}, {"name": "unfused", "fn": f_unfused}, {"name": "today", "fn": f_today},
                         {"name": "matmul", "fn": f_matmul}]
                time_sides(sides, args.rounds, args.window_ms)
                fm, um = report({"what": "glu", "n": n, "k": k, "m": m, "map": name}, sides, 4.0 * m * n * k, same)
                gate_rows.append({"m": m, "row": f"{n}x{k} {name}", "fused_median": fm, "unfused_min": um, "same": same})
                del sides, fcalls, ucalls, tcalls
            del dgs, dus, qgs, qus, dg, du, qg, qu
            torch.cuda.empty_cache()
        del wg, wu

    # ---- grouped
    gfentry, gwentry = hb._entry("mtq_packed_glu_wide_grouped"), hb._entry("mtq_packed_linear_wide_grouped")
    for shape in (s for s in args.grouped_shapes.split(",") if s):
        n, k = (int(v) for v in shape.split("x"))
        th, tw = hb.tiles_hw(n, k)
        for count in (int(v) for v in args.counts.split(",")):
            g = torch.Generator(device="cuda").manual_seed(args.seed + n + count)
            batches = []
            for side in range(2):
                w = torch.empty((count, n, k), dtype=torch.bfloat16, device="cuda")
                for e in range(count):
                    w[e] = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
                maps = np.random.default_rng(args.seed + count + side).choice(np.array([1, 2], dtype=np.int8), size=(count, th, tw), p=[0.85, 0.15])
                batches.append(packed.batch_of(packed.pack_batch(w, maps, backend="hip")))
                del w
            gb, ub = batches
            for kind in args.routings.split(","):
                per = prefill_routing(kind, count, args.seed)
                gr = np.concatenate([[0], np.cumsum(per)])
                T = int(gr[-1])
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
                grd = torch.from_numpy(gr.astype(np.int32)).cuda()
                yf, yu, yt, g16, u16 = (torch.zeros((T, n), dtype=torch.bfloat16, device="cuda") for _ in range(5))
                g32, u32 = (torch.zeros((T, n), dtype=torch.float32, device="cuda") for _ in range(2))
                need = hb.packed_glu_wide_grouped_workspace_bytes(T, count, n, k)
                ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
                tabs = [(b.arena.data_ptr(), b.arena.numel(), b.maps_dev.data_ptr(), b.offsets_dev.data_ptr(), b.bases_dev.data_ptr()) for b in (gb, ub)]
                hb.packed_glu_wide_grouped(x, grd, (gb.arena, gb.maps_dev, gb.offsets_dev, gb.bases_dev), (ub.arena, ub.maps_dev, ub.offsets_dev, ub.bases_dev),
                                           count, n, out_dtype=torch.bfloat16, out=yf, workspace=ws)     # the wrapper's checks, once
                fcall = (x.data_ptr(), T, k, k, grd.data_ptr(), *tabs[0], *tabs[1], count, n, None, None, 0, silu, yf.data_ptr(), bf16, n, ws.data_ptr(), need, stream)

                def wide(tab, out, code):
                    return (x.data_ptr(), T, k, k, grd.data_ptr(), *tab, count, n, None, 0, out.data_ptr(), code, n, ws.data_ptr(), need, stream)

                ucalls, tcalls = (wide(tabs[0], g32, f32), wide(tabs[1], u32, f32)), (wide(tabs[0], g16, bf16), wide(tabs[1], u16, bf16))
                ccall = (g32.data_ptr(), n, u32.data_ptr(), n, T, n, silu, yu.data_ptr(), bf16, n, stream)

                def f_fused(i):
                    hb.check(gfentry(*fcall))

                def f_unfused(i):
                    hb.check(gwentry(*ucalls[0]))
                    hb.check(gwentry(*ucalls[1]))
                    hb.check(centry(*ccall))

                def f_today(i):
                    hb.check(gwentry(*tcalls[0]))
                    hb.check(gwentry(*tcalls[1]))
                    torch.nn.functional.silu(g16, inplace=True)
                    torch.mul(g16, u16, out=yt)

                f_fused(0)
                f_unfused(0)
                torch.cuda.synchronize()
                same = bool(torch.equal(yf.view(torch.int16), yu.view(torch.int16)))
                say(f"## grouped {n}x{k} count={count} routing={kind}: T={T}, rows per expert min {int(per.min())} median {int(np.median(per))} max "
                    f"{int(per.max())}, {(gb.arena.numel() + ub.arena.numel()) / 1e6:.0f} MB of streams; fused bits {'equal to' if same else 'DIFFER from'} unfused")
                sides = [{"name": "fused", "fn": f_fused}, {"name": "unfused", "fn": f_unfused}, {"name": "today", "fn": f_today}]
                time_sides(sides, args.rounds, args.window_ms)
                report({"what": "glu_grouped", "n": n, "k": k, "count": count, "routing": kind, "T": T}, sides, 4.0 * T * n * k, same)
                del sides, x, yf, yu, yt, g16, u16, g32, u32
            del batches, gb, ub
            torch.cuda.empty_cache()

    # ---- the gate, from this run's dense rows alone
    if gate_rows:
        say("## the rule of packed.AUTO_GLU_FUSED_MIN_M, from this run's dense rows alone")
        say(f"bits: fused equal to unfused at every dense row: {all(r['same'] for r in gate_rows)}")
        ms = sorted({r["m"] for r in gate_rows})
        wins = {}
        for m in ms:
            at = [r for r in gate_rows if r["m"] == m]
            wins[m] = all(r["fused_median"] < r["unfused_min"] for r in at)
            worst = max(at, key=lambda r: r["fused_median"] / r["unfused_min"])
            say(f"m={m:5d}: fused median below the unfused minimum at {sum(r['fused_median'] < r['unfused_min'] for r in at)} of {len(at)} rows; the worst "
                f"ratio {worst['fused_median'] / worst['unfused_min']:6.3f} at {worst['row']}")
        gate = next((m for i, m in enumerate(ms) if all(wins[v] for v in ms[i:])), None)
        say(f"AUTO_GLU_FUSED_MIN_M by the rule: {gate}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
