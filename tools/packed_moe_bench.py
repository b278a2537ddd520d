"""The MoE routing entries (mtq_moe_plan, mtq_moe_dispatch, mtq_moe_combine) and packed.PackedMoE against the torch glue a user writes
without them, by the method of DESIGN.md §A.6g: device events after a warm-up, the sides alternated in one process, --rounds rounds of a
window each, medians and minima, the C entries called directly with prebuilt arguments.

  plan      ours   : mtq_moe_plan (one launch up to 1024 slots, three above);
            torch  : a stable argsort of the flat ids, bincount, cumsum into an int32 group_rows, and the inverse permutation;
  dispatch  ours   : mtq_moe_dispatch;                 torch: index_select of x by order // K;
  combine   ours   : mtq_moe_combine, float32 rows of the experts into bf16;
            torch  : index_select of the rows by the inverse permutation, times the weights, reshape, sum over K, to bf16;
  layer     ours   : PackedMoE.forward;                torch: the same module's experts between the torch glue above.

Shapes: count = 256, K = 8, k = n = 7168 (DeepSeek-R1; hidden 2048) and count = 8, K = 2, k = n = 4096 (Mixtral; hidden 14336), T in
--tokens.  The ids are torch.topk of random logits (int64), the weights their softmax.  For dispatch and combine the fraction of the
--hbm-tbs roofline on their own bytes, 2 * S * k * 2 and S * n * 4 + T * n * 2, from the median.  The plans are compared word for word
and the layers' outputs by their largest difference (torch sums the K terms in its own order) before any timing.

  python tools/packed_moe_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_moe.txt] [--json out.json] [--no-layer]
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
from tools.packed_glu_bench import time_sides

SHAPES = {"deepseek-r1": (256, 8, 7168, 2048), "mixtral": (8, 2, 4096, 14336)}   # count, K, k = n, hidden


def torch_plan(ids, count: int):
    """(order, group_rows int32, row_of) of (T, K) ids without drops."""
    flat = ids.reshape(-1)
    order = torch.argsort(flat, stable=True)
    group_rows = torch.zeros((count + 1,), dtype=torch.int32, device=ids.device)
    group_rows[1:] = torch.cumsum(torch.bincount(flat, minlength=count), 0)
    row_of = torch.empty_like(order)
    row_of[order] = torch.arange(order.numel(), device=ids.device)
    return order, group_rows, row_of


def torch_combine(ys, row_of, w, T: int, K: int):
    return (ys.index_select(0, row_of).view(T, K, -1) * w.unsqueeze(-1)).sum(1).to(torch.bfloat16)


def experts_of(count: int, k: int, hidden: int, seed: int):
    """Three device batches of `count` experts, all-bfp8 maps (the routing's cost does not depend on the maps)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    batches = []
    for rows, cols in ((hidden, k), (hidden, k), (k, hidden)):
        th, tw = hb.tiles_hw(rows, cols)
        w = torch.empty((count, rows, cols), dtype=torch.bfloat16, device="cuda")
        for e in range(count):
            w[e] = (torch.randn((rows, cols), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        batches.append(packed.batch_of(packed.pack_batch(w, np.full((count, th, tw), 1, dtype=np.int8), backend="hip")))
        del w
        torch.cuda.empty_cache()
    return batches


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--models", default="deepseek-r1,mixtral")
    p.add_argument("--tokens", default="1,8,32,512,4096")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--no-layer", action="store_true", help="skip the end-to-end rows (they pack the experts of a whole layer)")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines = [], []
    plan_fn, dispatch_fn, combine_fn = (hb._entry(name) for name in ("mtq_moe_plan", "mtq_moe_dispatch", "mtq_moe_combine"))

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides, nbytes=None):
        torch_min = min(sides[1]["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            row = {**label, "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3, "over_torch_min": med / torch_min}
            roof = ""
            if nbytes is not None:
                row["hbm_fraction"] = nbytes / (med * 1e-3) / (args.hbm_tbs * 1e12)
                roof = f"  {row['hbm_fraction'] * 100:5.1f}% of {args.hbm_tbs:g} TB/s on {nbytes / 1e6:8.2f} MB"
            rows_out.append(row)
            say(f"{s['name']:6s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  /torch-min {med / torch_min:6.3f}{roof}")

    say(f"# MoE routing on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, sides "
        f"alternated; int64 ids from topk, float32 expert rows, bf16 output; seed {args.seed}")
    for model in (m for m in args.models.split(",") if m):
        count, K, k, hidden = SHAPES[model]
        n = k
        moe = None
        if not args.no_layer:
            moe = packed.PackedMoE(*experts_of(count, k, hidden, args.seed), decode_max_rows=256)
        g = torch.Generator(device="cuda").manual_seed(args.seed + count)
        for T in (int(v) for v in args.tokens.split(",")):
            S = T * K
            logits = torch.randn((T, count), generator=g, device="cuda")
            top = torch.topk(logits, K, dim=-1)
            ids, w = top.indices.contiguous(), torch.softmax(top.values, dim=-1).float().contiguous()
            x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
            ys = torch.randn((S, n), generator=g, device="cuda")
            need = hb.moe_plan_workspace_bytes(T, K, count)
            ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
            plan = packed.moe_plan(ids, count, workspace=ws)                    # the wrapper's checks, once
            order, group_rows_t, row_of_t = torch_plan(ids, count)
            same = bool(torch.equal(plan.src.long(), order) and torch.equal(plan.group_rows, group_rows_t) and torch.equal(plan.row_of.long(), row_of_t))
            xs, xs_t = packed.moe_dispatch(x, plan), x.index_select(0, torch.div(order, K, rounding_mode="floor"))
            y = packed.moe_combine(ys, w, plan, out_dtype="bfloat16")
            y_t = torch_combine(ys, row_of_t, w, T, K)
            diff = float((y.float() - y_t.float()).abs().max())
            say(f"## {model}: count={count} K={K} k=n={k} T={T} (S={S}): plan words {'equal to' if same else 'DIFFER from'} torch's; dispatch "
                f"{'equal' if torch.equal(xs, xs_t) else 'DIFFERS'}; combine max abs diff to torch {diff:.3e}")
            pcall = (ids.data_ptr(), hb.IDS_I64, K, T, K, count, plan.group_rows.data_ptr(), plan.row_of.data_ptr(), plan.src.data_ptr(), ws.data_ptr(),
                     need, stream)
            dcall = (x.data_ptr(), T, k, k, plan.src.data_ptr(), K, xs.data_ptr(), k, stream)
            ccall = (ys.data_ptr(), hb.DTYPE_F32, n, plan.row_of.data_ptr(), w.data_ptr(), K, None, 0, 0, T, K, n, y.data_ptr(), hb.DTYPE_BF16, n, stream)
            src_rows = torch.div(order, K, rounding_mode="floor")
            label = {"model": model, "count": count, "K": K, "k": k, "T": T}
            for what, ours, theirs, nbytes in (
                    ("plan", lambda i: hb.check(plan_fn(*pcall)), lambda i: torch_plan(ids, count), None),
                    ("dispatch", lambda i: hb.check(dispatch_fn(*dcall)), lambda i: torch.index_select(x, 0, src_rows, out=xs_t), 2 * S * k * 2),
                    ("combine", lambda i: hb.check(combine_fn(*ccall)), lambda i: torch_combine(ys, row_of_t, w, T, K), S * n * 4 + T * n * 2)):
                sides = [{"name": "ours", "fn": ours}, {"name": "torch", "fn": theirs}]
                time_sides(sides, args.rounds, args.window_ms)
                say(f"### {what}")
                report({**label, "what": what}, sides, nbytes)
            if moe is not None:
                def layer_torch(i):
                    o, gr, ro = torch_plan(ids, count)
                    h = moe.experts(x.index_select(0, torch.div(o, K, rounding_mode="floor")), gr)
                    return torch_combine(h, ro, w, T, K)

                a, b = moe(x, ids, w), layer_torch(0)
                say(f"### layer (hidden {hidden}, all-bfp8 experts, decode_max_rows 256): max abs diff to the torch glue "
                    f"{float((a.float() - b.float()).abs().max()):.3e}")
                sides = [{"name": "ours", "fn": lambda i: moe(x, ids, w)}, {"name": "torch", "fn": layer_torch}]
                time_sides(sides, args.rounds, args.window_ms)
                report({**label, "what": "layer"}, sides)
            del x, ys, xs, xs_t, y, y_t
        del moe
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
