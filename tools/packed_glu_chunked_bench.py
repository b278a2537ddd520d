"""The grouped skinny GLU and the MoE decode route with a wave per 32-row chunk (include/mtq_glu_chunked.h) against the walking entries,
by the method of DESIGN.md §A.6r: device events after a warm-up, the sides alternated in one process, --rounds rounds of a window each,
medians and minima, the C entries called directly with prebuilt arguments, bf16 output, the bits compared before any timing.

  GLU rows      tools/packed_glu_bench.py --decode's six grouped rows: --counts experts of 2048 x 7168 under the 85 / 15 mix of bfp8 and
                bfp4, routings `one` (a row in every expert), `eight32` (8 rows in each of 32 experts) and `skew`, in both orientations.
                Sides: walk (mtq_packed_glu_skinny_grouped), chunks (mtq_packed_glu_skinny_grouped_chunked), wide
                (mtq_packed_glu_wide_grouped), each at the library's split; the matmul twins for the (k, n) orientation.
  combine rows  the same routings on 7168 x 2048 down experts: the walking and the chunked *_combine entries, S = T slots of 8 a token.
  layer rows    PackedMoE on --layer-count experts, K = 8, T = 32 and 64 tokens with a skewed id draw: decode_route x decode_grouped_kernel.

The run ends with the rule of packed.GLU_SKINNY_GROUPED_AUTO_KERNEL (DESIGN.md §A.6m's) applied to its own GLU and combine rows:
"chunks" only if on every skew row its median is below the walking entry's minimum, and on every uniform row (`one`, `eight32`) its
median is no more than the walk's minimum times the run's own spread, the largest median-to-minimum ratio of any side.

  python tools/packed_glu_chunked_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_glu_skinny_chunked.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tools.packed_glu_bench import decode_routing, time_sides

ROUTINGS = ("one", "eight32", "skew")


def _tabs(b):
    return b.arena.data_ptr(), b.arena.numel(), b.maps_dev.data_ptr(), b.offsets_dev.data_ptr(), b.bases_dev.data_ptr()


def _batch(w, maps, kn):
    pts = packed.pack_batch_transposed(w, maps, backend="hip") if kn else packed.pack_batch(w, maps, backend="hip")
    return packed.batch_to_device(packed.as_batch(pts))


def _maps(count, rows, cols, seed):
    th, tw = hb.tiles_hw(rows, cols)
    return np.random.default_rng(seed).choice(np.array([1, 2], dtype=np.int8), size=(count, th, tw), p=[0.85, 0.15])


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--counts", default="64,256")
    p.add_argument("--shape", default="2048x7168", help="hidden x model: the gate and up experts; the down experts are its transpose")
    p.add_argument("--layer-count", type=int, default=256)
    p.add_argument("--layer-tokens", default="32,64")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    silu, bf16, f32 = hb.ACT_CODE["silu"], hb.DTYPE_BF16, hb.DTYPE_F32
    lines, rule_rows, spreads = [], [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(what, row, kind, sides, same):
        walk_min = min(sides[0]["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            spreads.append(med / mn)
            say(f"{s['name']:8s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  /walk-min {med / walk_min:6.3f}")
        if what != "layer":
            rule_rows.append({"row": row, "kind": kind, "chunks_median": statistics.median(sides[1]["ts"]), "walk_min": walk_min, "same": same})

    say(f"# grouped skinny GLU and MoE decode, a wave per 32-row chunk, on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of "
        f"~{args.window_ms:.0f} ms windows, sides alternated; bf16 output; the library's split; seed {args.seed}")
    n, k = (int(v) for v in args.shape.split("x"))
    counts = [int(v) for v in args.counts.split(",")]
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    w_up = (torch.randn((max(counts + [args.layer_count]), n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    w_down = (torch.randn((max(counts + [args.layer_count]), k, n), generator=g, device="cuda") * 0.02).to(torch.bfloat16)

    for kn in (False, True):
        names = ("mtq_packed_glu_matmul_skinny_grouped", "mtq_packed_glu_matmul_skinny_grouped_chunked", "mtq_packed_glu_matmul_wide_grouped",
                 "mtq_packed_matmul_skinny_grouped_combine", "mtq_packed_matmul_skinny_grouped_chunked_combine") if kn else \
                ("mtq_packed_glu_skinny_grouped", "mtq_packed_glu_skinny_grouped_chunked", "mtq_packed_glu_wide_grouped",
                 "mtq_packed_linear_skinny_grouped_combine", "mtq_packed_linear_skinny_grouped_chunked_combine")
        walk, chunks, wide, cwalk, cchunks = (hb._entry(name) for name in names)
        orient = "(k, n)" if kn else "(n, k)"
        for count in counts:
            shape_up, shape_down = ((k, n), (n, k)) if kn else ((n, k), (k, n))
            gb = _batch(w_up[:count], _maps(count, *shape_up, args.seed + count), kn)
            ub = _batch(w_up[:count], _maps(count, *shape_up, args.seed + count + 1), kn)
            db = _batch(w_down[:count], _maps(count, *shape_down, args.seed + count + 2), kn)
            for kind in ROUTINGS:
                per = decode_routing(kind, count, args.seed)
                gr = np.concatenate([[0], np.cumsum(per)])
                T = int(gr[-1])
                grd = torch.from_numpy(gr.astype(np.int32)).cuda()
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
                ys = [torch.zeros((T, n), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
                need_w = hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, 0)
                need_c = hb.glu_grouped_chunked_workspace_bytes(T, count, n, k, 0, kn=kn)
                need_x = (hb.packed_glu_matmul_wide_grouped_workspace_bytes if kn else hb.packed_glu_wide_grouped_workspace_bytes)(T, count, n, k)
                wss = [torch.empty((max(v, 16),), dtype=torch.uint8, device="cuda") for v in (need_w, need_c, need_x)]
                head = (x.data_ptr(), T, k, k, grd.data_ptr(), *_tabs(gb), *_tabs(ub), count, n, None, None, 0, silu)
                calls = [(*head, ys[0].data_ptr(), bf16, n, 0, wss[0].data_ptr(), need_w, stream),
                         (*head, ys[1].data_ptr(), bf16, n, 0, wss[1].data_ptr(), need_c, stream),
                         (*head, ys[2].data_ptr(), bf16, n, wss[2].data_ptr(), need_x, stream)]
                sides = [{"name": name, "fn": (lambda i, fn=fn, call=call: hb.check(fn(*call)))}
                         for name, fn, call in zip(("walk", "chunks", "wide"), (walk, chunks, wide), calls)]
                for s in sides:
                    s["fn"](0)
                torch.cuda.synchronize()
                same = bool(torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)))          # before any timing
                row = f"glu {orient} {n}x{k} count={count} {kind}"
                say(f"## {row}: T={T}, rows per expert min {int(per.min())} median {int(np.median(per))} max {int(per.max())}, split "
                    f"{need_w // (8 * T * n)}; chunks bits {'equal to' if same else 'DIFFER from'} the walk's")
                time_sides(sides, args.rounds, args.window_ms)
                report("glu", row, kind, sides, same)

                # the down projection with the combine: h (S, n) -> y (tokens, k), S = T slots of 8 a token
                topk = 8
                tokens = T // topk
                h = torch.randn((T, n), generator=g, device="cuda").to(torch.bfloat16)
                row_of = torch.from_numpy(np.random.default_rng(args.seed + T).permutation(T).astype(np.int32)).cuda()
                wts = torch.rand((tokens, topk), generator=g, device="cuda")
                outs = [torch.zeros((tokens, k), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
                needs = [hb.moe_down_combine_workspace_bytes(T, count, k, n, 0, kn=kn, kernel=kernel) for kernel in ("walk", "chunks")]
                cws = [torch.empty((v,), dtype=torch.uint8, device="cuda") for v in needs]
                ccalls = [(h.data_ptr(), n, n, grd.data_ptr(), *_tabs(db), count, k, f32, row_of.data_ptr(), wts.data_ptr(), topk, None, 0, 0, tokens,
                           topk, out.data_ptr(), bf16, k, 0, ws.data_ptr(), need, stream) for out, ws, need in zip(outs, cws, needs)]
                sides = [{"name": name, "fn": (lambda i, fn=fn, call=call: hb.check(fn(*call)))}
                         for name, fn, call in zip(("walk", "chunks"), (cwalk, cchunks), ccalls)]
                for s in sides:
                    s["fn"](0)
                torch.cuda.synchronize()
                same = bool(torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)))
                row = f"combine {orient} {k}x{n} count={count} {kind}"
                say(f"## {row}: S={T}, {tokens} tokens of {topk}, split {needs[0] // (4 * T * k)}; chunks bits "
                    f"{'equal to' if same else 'DIFFER from'} the walk's")
                time_sides(sides, args.rounds, args.window_ms)
                report("combine", row, kind, sides, same)
                del sides, calls, ccalls, x, h, ys, outs, wss, cws
            del gb, ub, db
            torch.cuda.empty_cache()

    # ---- the layer: (n, k) experts, a skewed id draw, every combination of route and kernel
    count, topk = args.layer_count, 8
    gates = _batch(w_up[:count], _maps(count, n, k, args.seed + 7), False)
    ups = _batch(w_up[:count], _maps(count, n, k, args.seed + 8), False)
    downs = _batch(w_down[:count], _maps(count, k, n, args.seed + 9), False)
    rng = np.random.default_rng(args.seed)
    pr = rng.pareto(0.6, size=count) + 1e-3
    for T in (int(v) for v in args.layer_tokens.split(",")):
        ids = torch.from_numpy(np.stack([rng.choice(count, size=topk, replace=False, p=pr / pr.sum()) for _ in range(T)]).astype(np.int32)).cuda()
        per = np.bincount(ids.cpu().numpy().reshape(-1), minlength=count)
        x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
        wts = torch.rand((T, topk), generator=g, device="cuda")
        sides, outs = [], []
        for route in packed.MOE_DECODE_ROUTES:
            for kernel in ("walk", "chunks"):
                moe = packed.PackedMoE(gates, ups, downs, decode_max_rows=T * topk, max_tokens=T, decode_route=route, decode_grouped_kernel=kernel)
                outs.append(moe(x, ids, wts))
                sides.append({"name": f"{route[:6]}/{kernel}", "fn": (lambda i, moe=moe: moe(x, ids, wts))})
        torch.cuda.synchronize()
        same = all(torch.equal(o.view(torch.int16), outs[0].view(torch.int16)) for o in outs)
        say(f"## layer {count} experts {k} -> {n} -> {k}, T={T} K={topk}: rows per expert max {int(per.max())}, experts with rows "
            f"{int((per > 0).sum())}; the four modules' bits {'equal' if same else 'DIFFER'}")
        time_sides(sides, args.rounds, args.window_ms)
        report("layer", f"layer T={T}", "skew", sides, same)
        del sides, outs

    spread = max(spreads)
    say(f"## the rule for GLU_SKINNY_GROUPED_AUTO_KERNEL; the run's spread (largest median / minimum of any side): {spread:6.3f}")
    say(f"bits: chunks equal to the walk at every row: {all(r['same'] for r in rule_rows)}")
    fails = []
    for r in rule_rows:
        ratio = r["chunks_median"] / r["walk_min"]
        ok = ratio < 1.0 if r["kind"] == "skew" else ratio <= spread
        say(f"{'ok  ' if ok else 'FAIL'} {r['row']}: chunks median / walk minimum {ratio:6.3f} ({'below 1' if r['kind'] == 'skew' else f'at most {spread:5.3f}'})")
        if not ok:
            fails.append(r["row"])
    say(f'"auto" means {"chunks" if not fails else "walk"}' + ("" if not fails else f": decided by {len(fails)} row(s): " + "; ".join(fails)))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
