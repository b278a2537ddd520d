"""The gated product on packed (k, n) weights (mtq_packed_glu_matmul_wide / _skinny and their grouped forms) against the routes that exist
without them, by the method of DESIGN.md §A.6g as tools/packed_glu_bench.py applies it: bits first, then device events after a warm-up,
the sides alternated in one process, --rounds rounds of a window each, medians and minima, the C entries called directly with prebuilt
arguments, bf16 output, silu, and every side rotating over enough copies of the weights (--cold-mb in all) that a call does not find the
previous call's weights in the 256 MiB Infinity Cache.

Single tensor, hidden n x contraction k in --shapes, m in --ms, maps all-bfp8 and the 85 / 15 mix of bfp8 and bfp4:
  m <= 32   fused    : mtq_packed_glu_matmul_skinny at split 0, two launches;
            unfused  : THE YARDSTICK, the parent's kernels: two mtq_packed_matmul_skinny calls into float32 and mtq_glu_combine, five
                       launches, what glu_matmul(kernel="auto") runs there: the same bits as fused;
            linear   : mtq_packed_glu_skinny on the row-layout (n, k) packing of the same weights under the transposed maps (the same
                       bytes to read, other values: its groups run along k), for information;
  m > 32    fused    : mtq_packed_glu_matmul_wide, one launch;
            unfused  : THE YARDSTICK: two mtq_packed_matmul_wide calls into float32 and the combine (the faster of the parent's two
                       (k, n) kernels from m = 64 on, the block kernel's bits, so the same bits as fused);
            block    : two mtq_packed_matmul calls into float32 and the combine: glu_matmul(kernel="unfused");
            linear   : mtq_packed_glu_wide on the row-layout packing.
Grouped, --counts experts of --grouped-shape, --rows rows per expert, the mix: up to 32 rows per expert mtq_packed_glu_matmul_skinny_grouped
against two mtq_packed_matmul_skinny_grouped calls and the combine; from 32 on mtq_packed_glu_matmul_wide_grouped against two
mtq_packed_matmul_wide_grouped calls and the combine.
PackedMoE(stored="transpose").forward against the loop a user has to write without it (torch sort of the slots, a host read of the
counts, per expert packed.glu_matmul and packed.matmul, index_add_ of the weighted rows), --moe-experts experts, top-8, --moe-tokens tokens.

The run ends with the rules of packed.AUTO_GLU_MATMUL_SKINNY_MAX_M / AUTO_GLU_MATMUL_FUSED_MIN_M applied to its own single-tensor rows.

  python tools/packed_glu_matmul_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_glu_matmul.txt] [--json out.json]
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
from tools.packed_glu_bench import mixed_map, time_sides


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--cold-mb", type=float, default=640.0, help="rotate over copies of the two weights worth this many MB")
    p.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336", help="hidden n x contraction k")
    p.add_argument("--ms", default="1,8,32,64,128,512,4096")
    p.add_argument("--grouped-shape", default="2048x7168")
    p.add_argument("--counts", default="64,256")
    p.add_argument("--rows", default="1,4,32,128,512", help="rows per expert of the grouped rows")
    p.add_argument("--moe-experts", type=int, default=64)
    p.add_argument("--moe-tokens", default="16,1024")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines, gate_rows = [], [], []
    silu, bf16, f32 = hb.ACT_CODE["silu"], hb.DTYPE_BF16, hb.DTYPE_F32

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides, same):
        """sides[0] is the new route, sides[1] the yardstick."""
        base_min = min(sides[1]["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            rows_out.append({**label, "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3, "over_yardstick_min": med / base_min,
                             "bits_equal_yardstick": same})
            say(f"{s['name']:10s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  /{sides[1]['name']}-min {med / base_min:6.3f}")
        return statistics.median(sides[0]["ts"]), base_min

    def workspace(size):
        return torch.empty((max(size, 16),), dtype=torch.uint8, device="cuda")

    say(f"# packed gated product over (k, n) weights on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of "
        f"~{args.window_ms:.0f} ms windows, sides alternated; silu, bf16 output; weights rotated over {args.cold_mb:.0f} MB; seed {args.seed}")
    e_wide, e_skinny, e_mm, e_mmw, e_mms, e_comb, e_lw, e_ls = (hb._entry(name) for name in (
        "mtq_packed_glu_matmul_wide", "mtq_packed_glu_matmul_skinny", "mtq_packed_matmul", "mtq_packed_matmul_wide", "mtq_packed_matmul_skinny",
        "mtq_glu_combine", "mtq_packed_glu_wide", "mtq_packed_glu_skinny"))
    for shape in (s for s in args.shapes.split(",") if s):
        n, k = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(args.seed + n + k)
        wg, wu = ((torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(2))     # (n, k) as stored
        tkh, tnw = hb.tiles_hw(k, n)
        for name, mg, mu in (("bfp8", np.full((tkh, tnw), 1, dtype=np.int8), np.full((tkh, tnw), 1, dtype=np.int8)),
                             ("mix", mixed_map(tkh, tnw, args.seed), mixed_map(tkh, tnw, args.seed + 1))):
            tg, tu = hb.PackedTables.on_device(mg), hb.PackedTables.on_device(mu)                  # over the transpose's grid
            dg, du = hb.pack_tiles_transposed(wg, tg), hb.pack_tiles_transposed(wu, tu)            # the (k, n) streams
            rg, ru = hb.PackedTables.on_device(np.ascontiguousarray(mg.T)), hb.PackedTables.on_device(np.ascontiguousarray(mu.T))
            lg, lu = hb.pack_tiles(wg, rg), hb.pack_tiles(wu, ru)                                  # the row-layout (n, k) streams, the same formats
            copies = max(2, int(np.ceil(args.cold_mb * 1e6 / (tg.nbytes + tu.nbytes))))
            dgs, dus = [dg] + [dg.clone() for _ in range(copies - 1)], [du] + [du.clone() for _ in range(copies - 1)]
            lgs, lus = [lg] + [lg.clone() for _ in range(copies - 1)], [lu] + [lu.clone() for _ in range(copies - 1)]
            for m in (int(v) for v in args.ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                yf, yu, yb, yl = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(4))
                g32, u32 = (torch.empty((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
                ccall = (g32.data_ptr(), n, u32.data_ptr(), n, m, n, silu, None, bf16, n, stream)

                def glu_args(a, b, ta, tb, out):
                    return (x.data_ptr(), m, k, k, a.data_ptr(), ta.nbytes, ta.map_ptr, ta.offsets_ptr, b.data_ptr(), tb.nbytes, tb.map_ptr,
                            tb.offsets_ptr, n, None, None, silu, out.data_ptr(), bf16, n)

                def mm_args(a, ta, out):
                    return (x.data_ptr(), m, k, k, a.data_ptr(), ta.nbytes, ta.map_ptr, ta.offsets_ptr, n, None, out.data_ptr(), f32, n)

                def combine(out):
                    hb.check(e_comb(*ccall[:7], out.data_ptr(), *ccall[8:]))

                decode = m <= packed.SKINNY_MAX_M
                if decode:
                    need, need1 = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, 0), hb.packed_matmul_skinny_workspace_bytes(m, n, k, 0)
                    ws, wsl, wsg, wsu = workspace(need), workspace(need), workspace(need1), workspace(need1)
                    hb.packed_glu_matmul_skinny(x, dg, tg, du, tu, n, out_dtype=torch.bfloat16, out=yf)    # the wrapper's checks, once
                    fcalls = [glu_args(a, b, tg, tu, yf) + (0, ws.data_ptr(), need, stream) for a, b in zip(dgs, dus)]
                    lcalls = [glu_args(a, b, rg, ru, yl) + (0, wsl.data_ptr(), need, stream) for a, b in zip(lgs, lus)]
                    ucalls = [(mm_args(a, tg, g32) + (0, wsg.data_ptr() if need1 else None, need1, stream),
                               mm_args(b, tu, u32) + (0, wsu.data_ptr() if need1 else None, need1, stream)) for a, b in zip(dgs, dus)]
                    fentry, lentry, uentry = e_skinny, e_ls, e_mms
                else:
                    hb.packed_glu_matmul_wide(x, dg, tg, du, tu, n, out_dtype=torch.bfloat16, out=yf)      # the wrapper's checks, once
                    fcalls = [glu_args(a, b, tg, tu, yf) + (stream,) for a, b in zip(dgs, dus)]
                    lcalls = [glu_args(a, b, rg, ru, yl) + (stream,) for a, b in zip(lgs, lus)]
                    ucalls = [(mm_args(a, tg, g32) + (stream,), mm_args(b, tu, u32) + (stream,)) for a, b in zip(dgs, dus)]
                    fentry, lentry, uentry = e_wide, e_lw, e_mmw

                def f_fused(i):
                    hb.check(fentry(*fcalls[i % copies]))

                def f_linear(i):
                    hb.check(lentry(*lcalls[i % copies]))

                def f_unfused(i):
                    a, b = ucalls[i % copies]
                    hb.check(uentry(*a))
                    hb.check(uentry(*b))
                    combine(yu)

                def f_block(i):
                    a, b = ucalls[i % copies]
                    hb.check(e_mm(*a))
                    hb.check(e_mm(*b))
                    combine(yb)

                f_fused(0)
                f_unfused(0)
                f_linear(0)
                if not decode:
                    f_block(0)
                torch.cuda.synchronize()
                same = bool(torch.equal(yf.view(torch.int16), yu.view(torch.int16)))            # before any timing
                same_b = decode or bool(torch.equal(yf.view(torch.int16), yb.view(torch.int16)))
                err = float((yf.float() - yl.float()).abs().max() / yl.float().abs().max().clamp_min(1e-30))
                say(f"## {n}x{k} m={m} map={name}: fused bits {'equal to' if same else 'DIFFER from'} unfused"
                    + ("" if decode else f", {'equal to' if same_b else 'DIFFER from'} the block pair's")
                    + f"; max rel diff to the linear side {err:.2e} (its groups run along k, these along n: other quantised values)")
                sides = [{"name": "fused", "fn": f_fused}, {"name": "unfused", "fn": f_unfused}, {"name": "linear", "fn": f_linear}]
                if not decode:
                    sides.append({"name": "block", "fn": f_block})
                time_sides(sides, args.rounds, args.window_ms)
                fm, um = report({"what": "glu_matmul", "n": n, "k": k, "m": m, "map": name}, sides, same and same_b)
                gate_rows.append({"m": m, "row": f"{n}x{k} {name}", "fused_median": fm, "unfused_min": um, "same": same and same_b})
                del sides, fcalls, lcalls, ucalls
            del dgs, dus, lgs, lus, dg, du, lg, lu
            torch.cuda.empty_cache()
        del wg, wu

    # ---- grouped
    e_gw, e_gs, e_mgw, e_mgs = (hb._entry(name) for name in ("mtq_packed_glu_matmul_wide_grouped", "mtq_packed_glu_matmul_skinny_grouped",
                                                             "mtq_packed_matmul_wide_grouped", "mtq_packed_matmul_skinny_grouped"))
    n, k = (int(v) for v in args.grouped_shape.split("x"))
    tkh, tnw = hb.tiles_hw(k, n)
    grouped_rows = []
    for count in (int(v) for v in args.counts.split(",") if v):
        g = torch.Generator(device="cuda").manual_seed(args.seed + n + count)
        batches = []
        for side in range(2):
            w = torch.empty((count, n, k), dtype=torch.bfloat16, device="cuda")
            for e in range(count):
                w[e] = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            maps = np.random.default_rng(args.seed + count + side).choice(np.array([1, 2], dtype=np.int8), size=(count, tkh, tnw), p=[0.85, 0.15])
            batches.append(packed.batch_of(packed.pack_batch_transposed(w, maps, backend="hip")))
            del w
        gb, ub = batches
        tabs = [(b.arena.data_ptr(), b.arena.numel(), b.maps_dev.data_ptr(), b.offsets_dev.data_ptr(), b.bases_dev.data_ptr()) for b in (gb, ub)]
        sides_t = tuple((b.arena, b.maps_dev, b.offsets_dev, b.bases_dev) for b in (gb, ub))
        for per in (int(v) for v in args.rows.split(",")):
            T = per * count
            x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
            grd = torch.arange(0, T + 1, per, dtype=torch.int32, device="cuda")
            g32, u32 = (torch.zeros((T, n), dtype=torch.float32, device="cuda") for _ in range(2))
            for family in (("skinny",) if per < 32 else ("skinny", "wide") if per == 32 else ("wide",)):
                yf, yu = (torch.zeros((T, n), dtype=torch.bfloat16, device="cuda") for _ in range(2))
                head = (x.data_ptr(), T, k, k, grd.data_ptr())
                ccall = (g32.data_ptr(), n, u32.data_ptr(), n, T, n, silu, yu.data_ptr(), bf16, n, stream)
                if family == "skinny":
                    need, need1 = hb.packed_glu_matmul_skinny_grouped_workspace_bytes(T, count, n, k, 0), hb.packed_matmul_skinny_grouped_workspace_bytes(T, count, n, k, 0)
                    ws, ws1 = workspace(need), workspace(need1)
                    hb.packed_glu_matmul_skinny_grouped(x, grd, sides_t[0], sides_t[1], count, n, out_dtype=torch.bfloat16, out=yf, workspace=ws)
                    fcall = head + tabs[0] + tabs[1] + (count, n, None, None, 0, silu, yf.data_ptr(), bf16, n, 0, ws.data_ptr(), need, stream)
                    ucalls = [head + tab + (count, n, None, 0, out.data_ptr(), f32, n, 0, ws1.data_ptr() if need1 else None, need1, stream)
                              for tab, out in ((tabs[0], g32), (tabs[1], u32))]
                    fentry, uentry = e_gs, e_mgs
                else:
                    need = hb.packed_glu_matmul_wide_grouped_workspace_bytes(T, count, n, k)
                    ws = workspace(need)
                    hb.packed_glu_matmul_wide_grouped(x, grd, sides_t[0], sides_t[1], count, n, out_dtype=torch.bfloat16, out=yf, workspace=ws)
                    fcall = head + tabs[0] + tabs[1] + (count, n, None, None, 0, silu, yf.data_ptr(), bf16, n, ws.data_ptr(), need, stream)
                    ucalls = [head + tab + (count, n, None, 0, out.data_ptr(), f32, n, ws.data_ptr(), need, stream) for tab, out in ((tabs[0], g32), (tabs[1], u32))]
                    fentry, uentry = e_gw, e_mgw

                def f_fused(i):
                    hb.check(fentry(*fcall))

                def f_unfused(i):
                    hb.check(uentry(*ucalls[0]))
                    hb.check(uentry(*ucalls[1]))
                    hb.check(e_comb(*ccall))

                f_fused(0)
                f_unfused(0)
                torch.cuda.synchronize()
                same = bool(torch.equal(yf.view(torch.int16), yu.view(torch.int16)))
                say(f"## grouped {n}x{k} count={count} rows/expert={per} ({family}): T={T}, {(gb.arena.numel() + ub.arena.numel()) / 1e6:.0f} MB of "
                    f"streams; fused bits {'equal to' if same else 'DIFFER from'} unfused")
                sides = [{"name": "fused", "fn": f_fused}, {"name": "unfused", "fn": f_unfused}]
                time_sides(sides, args.rounds, args.window_ms)
                fm, um = report({"what": "glu_matmul_grouped", "n": n, "k": k, "count": count, "rows": per, "family": family}, sides, same)
                grouped_rows.append({"row": f"count={count} rows={per} {family}", "fused_median": fm, "unfused_min": um, "same": same})
                del sides, yf, yu
            del x, g32, u32
        del batches, gb, ub, tabs, sides_t
        torch.cuda.empty_cache()

    # ---- the layer
    moe_rows = []
    if args.moe_experts > 0:
        count, topk, k_out = args.moe_experts, 8, k
        g = torch.Generator(device="cuda").manual_seed(args.seed + 7)
        lists = []
        for rows_, cols_, seed in ((n, k, 1), (n, k, 2), (k_out, n, 3)):                 # gate, up (hidden, k) and down (k_out, hidden), as stored
            w = torch.empty((count, rows_, cols_), dtype=torch.bfloat16, device="cuda")
            for e in range(count):
                w[e] = (torch.randn((rows_, cols_), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            th, tw = hb.tiles_hw(cols_, rows_)
            maps = np.random.default_rng(args.seed + seed).choice(np.array([1, 2], dtype=np.int8), size=(count, th, tw), p=[0.85, 0.15])
            lists.append(packed.pack_batch_transposed(w, maps, backend="hip"))
            del w
        gates, ups, downs = lists
        for tokens in (int(v) for v in args.moe_tokens.split(",") if v):
            moe = packed.PackedMoE(gates, ups, downs, out_dtype="bfloat16", stored="transpose", decode_max_rows=32 * count, max_tokens=tokens)
            x = torch.randn((tokens, k), generator=g, device="cuda").to(torch.bfloat16)
            ids = torch.stack([torch.randperm(count, generator=g, device="cuda")[:topk] for _ in range(tokens)]).to(torch.int32)
            wts = torch.rand((tokens, topk), generator=g, device="cuda") + 0.25
            out = {}

            def f_layer(i):
                out["layer"] = moe(x, ids, wts)

            def f_loop(i):
                flat = ids.reshape(-1).long()
                order = torch.sort(flat, stable=True).indices
                per_e = torch.bincount(flat, minlength=count).cpu().tolist()               # the host read the loop cannot do without
                xs = x[order // topk]
                acc = torch.zeros((tokens, k_out), dtype=torch.float32, device="cuda")
                r0 = 0
                for e, c in enumerate(per_e):
                    if c:
                        h = packed.glu_matmul(xs[r0:r0 + c], gates[e], ups[e], out_dtype="bfloat16", kernel="auto")
                        y = packed.matmul(h, downs[e], kernel="auto")
                        sl = order[r0:r0 + c]
                        acc.index_add_(0, sl // topk, y * wts.reshape(-1)[sl][:, None])
                        r0 += c
                out["loop"] = acc.to(torch.bfloat16)

            f_layer(0)
            f_loop(0)
            torch.cuda.synchronize()
            err = float((out["layer"].float() - out["loop"].float()).abs().max() / out["loop"].float().abs().max().clamp_min(1e-30))
            say(f"## PackedMoE(stored=\"transpose\") {count} experts of {n}x{k}, top-{topk}, {tokens} tokens (S = {tokens * topk} rows): max rel diff "
                f"to the loop {err:.2e} (the loop sums in another order and family)")
            sides = [{"name": "layer", "fn": f_layer}, {"name": "loop", "fn": f_loop}]
            time_sides(sides, args.rounds, args.window_ms)
            fm, um = report({"what": "moe", "count": count, "tokens": tokens}, sides, err < 2e-2)
            moe_rows.append({"row": f"tokens={tokens}", "fused_median": fm, "unfused_min": um})
            del moe, sides
        del lists, gates, ups, downs
        torch.cuda.empty_cache()

    # ---- the gates, from this run's rows alone
    if gate_rows:
        say("## the rules of packed.AUTO_GLU_MATMUL_SKINNY_MAX_M and AUTO_GLU_MATMUL_FUSED_MIN_M, from this run's single-tensor rows alone")
        say(f"bits: fused equal to every other side at every row: {all(r['same'] for r in gate_rows)}")
        ms = sorted({r["m"] for r in gate_rows})
        wins = {}
        for m in ms:
            at = [r for r in gate_rows if r["m"] == m]
            wins[m] = all(r["fused_median"] < r["unfused_min"] for r in at)
            worst = max(at, key=lambda r: r["fused_median"] / r["unfused_min"])
            say(f"m={m:5d}: fused median below the yardstick's minimum at {sum(r['fused_median'] < r['unfused_min'] for r in at)} of {len(at)} rows; the "
                f"worst ratio {worst['fused_median'] / worst['unfused_min']:6.3f} at {worst['row']}")
        above = [m for m in ms if m > packed.SKINNY_MAX_M]
        gate = next((m for i, m in enumerate(above) if all(wins[v] for v in above[i:])), None)
        say(f"AUTO_GLU_MATMUL_FUSED_MIN_M by the rule: {gate} (the package has {packed.AUTO_GLU_MATMUL_FUSED_MIN_M})")
        below = [m for m in ms if m <= packed.SKINNY_MAX_M]
        say(f"glu_matmul_skinny (PackedMatmulMLP(decode_kernel=\"fused\")) wins at every row of m in {[m for m in below if wins[m]]}, not at "
            f"{[m for m in below if not wins[m]]}; glu_matmul(kernel=\"auto\") runs the yardstick there whatever this says")
    for title, rows_ in (("grouped", grouped_rows), ("PackedMoE", moe_rows)):
        lost = [r for r in rows_ if not r["fused_median"] < r["unfused_min"]]
        if rows_:
            say(f"## {title}: the new route's median is below the other side's minimum at {len(rows_) - len(lost)} of {len(rows_)} rows"
                + ("" if not lost else "; NOT at " + ", ".join(f"{r['row']} ({r['fused_median'] / r['unfused_min']:.3f})" for r in lost)))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
