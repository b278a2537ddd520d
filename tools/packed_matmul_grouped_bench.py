"""The grouped packed matmul for (k, n) experts (mtq_packed_matmul_skinny_grouped, _chunked, mtq_packed_matmul_wide_grouped) against the
routes that exist without it, by the method of tools/packed_grouped_bench.py (device events after a warm-up, sides
alternated in one process, --rounds rounds of a window each, medians and minima), whose helpers, shapes, counts, map mix and seeded
Pareto draw it uses.  The experts are `count` weights (n, k) packed in the transposed layout (pack_batch_transposed: (k, n) tensors, maps
over the transposes' grid) and, for (b), the same weights in the row layout under the transposed maps (pack_batch).

Decode routings (`even1`, `even4`, `even32`: that many rows per expert; `skew`: 512 rows by the seeded Pareto draw), all at split 0:
  walk, chunks : the two new skinny entries, workspaces allocated once;
  (a) loop     : mtq_packed_matmul_skinny per non-empty group and 32-row chunk at the library's own split for one expert, the C entry
                 with prebuilt arguments and one workspace - what a caller has without the grouped entries (for the bit check
                 the loop runs once more at the grouped entries' effective split);
  (b) linear   : mtq_packed_linear_skinny_grouped and _chunked on the row-layout arena: the cost of the [k][n] image;
  (c) matmul   : torch.matmul per non-empty group on the unpacked bf16 weights, for information.
Prefill routings (`even128`, `even512`):
  wide-grouped : the new wide entry;  (a) mtq_packed_matmul_wide per group;  (b) mtq_packed_linear_wide_grouped;  (c) as above.
Before any timing the new entries' bf16 outputs are compared bit for bit: walk with chunks and with (a); wide-grouped with (a).
The run ends with the rule of DESIGN.md §A.6m for MATMUL_GROUPED_AUTO_KERNEL, answered from this run's numbers alone.

  python tools/packed_matmul_grouped_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_matmul_grouped.txt] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tools.packed_grouped_bench import calibrate, routing, window_ms

DECODE = {"even1": 1, "even4": 4, "even32": 32}
PREFILL = {"even128": 128, "even512": 512}


def rows_per_expert(kind: str, count: int, seed: int) -> np.ndarray:
    if kind in DECODE or kind in PREFILL:
        return np.full(count, {**DECODE, **PREFILL}[kind], dtype=np.int64)
    if kind == "skew":
        return routing("sparse", count, seed)
    raise SystemExit(f"unknown routing {kind!r}")


def commit() -> str:
    try:
        root = Path(__file__).resolve().parents[1]
        head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "status", "--porcelain"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
        return head + (" with uncommitted changes (the tree this tool is part of)" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git metadata beside the tree)"


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--shapes", default="2048x7168,7168x2048")
    p.add_argument("--counts", default="64,256")
    p.add_argument("--routings", default="even1,even4,even32,skew,even128,even512")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--commit", default=None, help="the commit measured, when the tree has no git metadata beside it")
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

    say(f"# grouped packed matmul on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"sides alternated; bf16 output; maps 85% bfp8 / 15% bfp4; seed {args.seed}; commit {args.commit or commit()}")
    E = {name: hb._entry("mtq_packed_" + name) for name in (
        "matmul_skinny_grouped", "matmul_skinny_grouped_chunked", "matmul_wide_grouped", "matmul_skinny", "matmul_wide",
        "linear_skinny_grouped", "linear_skinny_grouped_chunked", "linear_wide_grouped")}
    BF = hb.DTYPE_BF16
    for shape in args.shapes.split(","):
        n, k = (int(v) for v in shape.split("x"))
        tkh, tnw = hb.tiles_hw(k, n)
        for count in (int(v) for v in args.counts.split(",")):
            g = torch.Generator(device="cuda").manual_seed(args.seed + n + count)
            w = torch.empty((count, n, k), dtype=torch.bfloat16, device="cuda")
            for e in range(count):
                w[e] = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            maps_t = np.random.default_rng(args.seed + count).choice(np.array([1, 2], dtype=np.int8), size=(count, tkh, tnw), p=[0.85, 0.15])
            pts = packed.pack_batch_transposed(w, maps_t, backend="hip")                        # (k, n) experts
            rpts = packed.pack_batch(w, np.ascontiguousarray(maps_t.transpose(0, 2, 1)), backend="hip")   # (n, k): the same weights, the maps' transposes
            del w
            bt, br = packed.batch_of(pts), packed.batch_of(rpts)
            phat = packed.unpack_batch(pts, backend="hip", dtype="bfloat16")                     # (count, k, n)
            tab_t = (bt.arena.data_ptr(), bt.arena.numel(), bt.maps_dev.data_ptr(), bt.offsets_dev.data_ptr(), bt.bases_dev.data_ptr())
            tab_r = (br.arena.data_ptr(), br.arena.numel(), br.maps_dev.data_ptr(), br.offsets_dev.data_ptr(), br.bases_dev.data_ptr())
            for kind in args.routings.split(","):
                per = rows_per_expert(kind, count, args.seed)
                gr = np.concatenate([[0], np.cumsum(per)])
                T, active = int(gr[-1]), int((per > 0).sum())
                active_mb = sum(pts[e].nbytes for e in range(count) if per[e]) / 1e6
                prefill = kind in PREFILL
                say(f"## {n}x{k} (n x k) count={count} routing={kind}: T={T}, {active} experts with rows ({active_mb:.0f} MB of "
                    f"{bt.arena.numel() / 1e6:.0f} MB of streams), rows per expert min {int(per.min())} median {int(np.median(per))} max {int(per.max())}")
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
                grd = torch.from_numpy(gr.astype(np.int32)).cuda()
                ys = {name: torch.zeros((T, n), dtype=torch.bfloat16, device="cuda") for name in ("new", "new2", "loop", "lin", "lin2", "mm")}
                groups = [(e, int(gr[e]), int(gr[e + 1])) for e in range(count) if per[e]]

                def grouped(entry, tables, y, size, split):
                    """(the prebuilt call, its kept workspace) of a grouped entry; split None: a wide entry"""
                    need = size(T, count, n, k) if split is None else size(T, count, n, k, split)
                    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
                    call = (x.data_ptr(), T, k, k, grd.data_ptr(), *tables, count, n, None, 0, y.data_ptr(), BF, n,
                            *(() if split is None else (split,)), ws.data_ptr() if need else None, need, stream)
                    return (lambda: hb.check(entry(*call))), ws

                def f_matmul():
                    for e, r0, r1 in groups:
                        torch.matmul(x[r0:r1], phat[e], out=ys["mm"][r0:r1])

                keep = []
                if prefill:
                    f_new, ws = grouped(E["matmul_wide_grouped"], tab_t, ys["new"], hb.packed_matmul_wide_grouped_workspace_bytes, None)
                    f_lin, ws2 = grouped(E["linear_wide_grouped"], tab_r, ys["lin"], hb.packed_linear_wide_grouped_workspace_bytes, None)
                    keep += [ws, ws2]
                    lcalls = []
                    for e, r0, r1 in groups:
                        t = pts[e].tables()
                        lcalls.append((x[r0:r1].data_ptr(), r1 - r0, k, k, pts[e].data.data_ptr(), t.nbytes, t.map_ptr, t.offsets_ptr, n, None,
                                       ys["loop"][r0:r1].data_ptr(), BF, n, stream))

                    def f_loop():
                        for call in lcalls:
                            hb.check(E["matmul_wide"](*call))

                    sides = [{"name": "wide-grouped", "fn": f_new}, {"name": f"(a) loop of {len(lcalls)} matmul_wide", "fn": f_loop},
                             {"name": "(b) linear_wide_grouped, row layout", "fn": f_lin}, {"name": f"(c) loop of {len(groups)} matmuls", "fn": f_matmul}]
                else:
                    f_new, ws = grouped(E["matmul_skinny_grouped"], tab_t, ys["new"], hb.packed_matmul_skinny_grouped_workspace_bytes, 0)
                    f_new2, ws2 = grouped(E["matmul_skinny_grouped_chunked"], tab_t, ys["new2"], hb.packed_matmul_skinny_grouped_chunked_workspace_bytes, 0)
                    f_lin, ws3 = grouped(E["linear_skinny_grouped"], tab_r, ys["lin"], hb.packed_linear_skinny_grouped_workspace_bytes, 0)
                    f_lin2, ws4 = grouped(E["linear_skinny_grouped_chunked"], tab_r, ys["lin2"], hb.packed_linear_skinny_grouped_chunked_workspace_bytes, 0)
                    eff = max(1, hb.packed_matmul_skinny_grouped_workspace_bytes(T, count, n, k, 0) // (4 * T * n))
                    leff = max(1, hb.packed_matmul_skinny_workspace_bytes(32, n, k, 0) // (4 * 32 * n))    # the library's split of one expert
                    lneed = max(hb.packed_matmul_skinny_workspace_bytes(32, n, k, s) for s in (eff, leff))
                    lws = torch.empty((max(lneed, 16),), dtype=torch.uint8, device="cuda")
                    keep += [ws, ws2, ws3, ws4, lws]

                    def loop_calls(split):
                        calls = []
                        for e, r0, r1 in groups:
                            t = pts[e].tables()
                            for r in range(r0, r1, 32):
                                m = min(32, r1 - r)
                                calls.append((x[r:r + m].data_ptr(), m, k, k, pts[e].data.data_ptr(), t.nbytes, t.map_ptr, t.offsets_ptr, n, None,
                                              ys["loop"][r:r + m].data_ptr(), BF, n, split, lws.data_ptr(), lws.numel(), stream))
                        return calls

                    lcalls, ccalls = loop_calls(leff), loop_calls(eff)   # timed at the library's own split; the bits are checked at the grouped one

                    def f_loop():
                        for call in lcalls:
                            hb.check(E["matmul_skinny"](*call))

                    sides = [{"name": f"walk split=0 (eff {eff})", "fn": f_new}, {"name": "chunks split=0", "fn": f_new2},
                             {"name": f"(a) loop of {len(lcalls)} matmul_skinny, split {leff}", "fn": f_loop},
                             {"name": "(b) linear walk, row layout", "fn": f_lin}, {"name": "(b) linear chunks, row layout", "fn": f_lin2},
                             {"name": f"(c) loop of {len(groups)} matmuls", "fn": f_matmul}]
                for s in sides:                               # every side once, before any timing
                    s["fn"]()
                if not prefill:                               # the contract's loop: the single-tensor entry at the grouped entries' split
                    for call in ccalls:
                        hb.check(E["matmul_skinny"](*call))
                torch.cuda.synchronize()
                bits = lambda a, b: bool(torch.equal(ys[a].view(torch.int16), ys[b].view(torch.int16)))   # noqa: E731
                same = bits("new", "loop") and (prefill or bits("new", "new2"))
                scale = float(ys["mm"].float().abs().max().clamp_min(1e-30))
                say(f"{'bits':44s} the new entr{'y' if prefill else 'ies'} {'equal to' if same else 'DIFFER from'} the (a) loop"
                    f"{'' if prefill else ' and each other'}; max rel diff of the first to matmul {float((ys['new'].float() - ys['mm'].float()).abs().max()) / scale:.2e}")
                for s in sides:
                    s["iters"], s["ts"] = calibrate(s["fn"], args.window_ms), []
                for _ in range(args.rounds):
                    for s in sides:
                        s["ts"].append(window_ms(s["fn"], s["iters"]))
                torch.cuda.synchronize()
                med = {s["name"]: statistics.median(s["ts"]) for s in sides}
                mn = {s["name"]: min(s["ts"]) for s in sides}
                names = [s["name"] for s in sides]
                loop_min = mn[names[1 if prefill else 2]]
                for s in sides:
                    nm = s["name"]
                    rows_out.append({"n": n, "k": k, "count": count, "routing": kind, "T": T, "active": active, "side": nm, "ms_median": med[nm],
                                     "ms_min": mn[nm], "over_loop_min": med[nm] / loop_min, "same_bits": same})
                    say(f"{nm:44s} {med[nm] * 1e3:9.1f} us (min {mn[nm] * 1e3:9.1f}, spread {(med[nm] - mn[nm]) / med[nm] * 100:4.1f}%)  "
                        f"{active_mb / med[nm]:7.1f} GB/s of active streams  {2.0 * T * n * k / med[nm] / 1e9:7.1f} TFLOP/s  /(a)-min {med[nm] / loop_min:6.3f}")
                v = {"row": f"{n}x{k} count={count} {kind}", "prefill": prefill, "same": same,
                     "spread": max(med[nm] / mn[nm] for nm in names if not nm.startswith("(c)"))}
                if prefill:
                    v.update(new=med[names[0]], loop_min=loop_min, lin=med[names[2]], lin_min=mn[names[2]])
                else:
                    v.update(walk=med[names[0]], walk_min=mn[names[0]], chunks=med[names[1]], chunks_min=mn[names[1]], loop_min=loop_min,
                             lin_walk=med[names[3]], lin_chunks=med[names[4]], sparse=kind == "skew")
                verdict.append(v)
                del sides, lcalls, keep, x, ys, f_loop
            del pts, rpts, bt, br, phat
            torch.cuda.empty_cache()
    say("## summary, from this run alone")
    say(f"bits equal at every row: {all(v['same'] for v in verdict)}")
    for v in verdict:
        if v["prefill"]:
            say(f"{v['row']:34s} wide-grouped / (a) min {v['new'] / v['loop_min']:6.3f}   wide-grouped / (b) linear_wide_grouped {v['new'] / v['lin']:6.3f}")
        else:
            say(f"{v['row']:34s} walk / (a) min {v['walk'] / v['loop_min']:6.3f}  chunks / (a) min {v['chunks'] / v['loop_min']:6.3f}  "
                f"chunks / walk min {v['chunks'] / v['walk_min']:6.3f}  walk / (b) linear walk {v['walk'] / v['lin_walk']:6.3f}  "
                f"chunks / (b) linear chunks {v['chunks'] / v['lin_chunks']:6.3f}")
    dec = [v for v in verdict if not v["prefill"]]
    if dec:
        spread = max(v["spread"] for v in verdict)
        one = all(v["chunks"] < v["walk_min"] for v in dec if v["sparse"])
        two = all(v["chunks"] <= v["walk_min"] * spread for v in dec if not v["sparse"])
        say(f"the rule of DESIGN.md A.6m: (1) chunks' median below walk's minimum on every skewed row: {one}; (2) chunks' median within the "
            f"run's spread ({spread:.4f}) of walk's minimum on every even row: {two}  ->  MATMUL_GROUPED_AUTO_KERNEL = "
            f"{'chunks' if one and two else 'walk'!r}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
