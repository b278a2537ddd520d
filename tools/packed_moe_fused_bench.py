"""The decode route of packed.PackedMoE without its staging copies (decode_route="fused": the gather inside the gated product's X
loads, the combine inside the down projection's reduce) against the staged route of the same build, by the method of
tools/packed_moe_bench.py: device events after a warm-up, the sides alternated in one process, --rounds rounds of a window each,
medians and minima, the C entries called directly with prebuilt arguments.

  glu     fused : mtq_packed_glu_skinny_grouped_gather (2 launches);
          staged: mtq_moe_dispatch + mtq_packed_glu_skinny_grouped (3 launches), into bf16;
  down    fused : mtq_packed_linear_skinny_grouped_combine (2 launches);
          staged: mtq_packed_linear_skinny_grouped into float32 (1 launch, 2 when the split is above 1) + mtq_moe_combine, into bf16;
  layer   fused : PackedMoE(decode_route="fused").forward;   staged: PackedMoE(decode_route="staged").forward, the same experts.

Shapes: count = 256, K = 8, k = n = 7168 (DeepSeek-R1; hidden 2048) and count = 8, K = 2, k = n = 4096 (Mixtral; hidden 14336), T in
--tokens, all-bfp8 experts, decode_max_rows = 256, split 0 (the library's choice) on both sides.  The ids are torch.topk of random
logits (int64), the weights their softmax.  Every pair is compared bit for bit before it is timed.

  python tools/packed_moe_fused_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_moe_fused.txt] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tools.packed_glu_bench import time_sides
from tools.packed_moe_bench import SHAPES, experts_of


def arena_args(batch):
    return batch.arena.data_ptr(), batch.arena.numel(), batch.maps_dev.data_ptr(), batch.offsets_dev.data_ptr(), batch.bases_dev.data_ptr()


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--models", default="deepseek-r1,mixtral")
    p.add_argument("--tokens", default="1,8,32")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    rows_out, lines = [], []
    dispatch_fn, combine_fn, glu_fn, lin_fn = (hb._entry(name) for name in ("mtq_moe_dispatch", "mtq_moe_combine", "mtq_packed_glu_skinny_grouped",
                                                                          "mtq_packed_linear_skinny_grouped"))
    gather_fn, down_fn = hb._entry(hb.MOE_GATHER[0][0]), hb._entry(hb.MOE_DOWN_COMBINE[0][0])
    silu, bf16, f32 = hb.ACT_CODE["silu"], hb.DTYPE_BF16, hb.DTYPE_F32

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides, same):
        base_med, base_min = statistics.median(sides[1]["ts"]), min(sides[1]["ts"])
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            rows_out.append({**label, "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3, "over_staged_median": med / base_med,
                             "over_staged_min": med / base_min, "bits_equal_staged": same})
            say(f"{s['name']:6s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)  /staged-median {med / base_med:6.3f}"
                f"  /staged-min {med / base_min:6.3f}")

    say(f"# MoE decode, fused against staged, on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms "
        f"windows, sides alternated; int64 ids from topk, all-bfp8 experts, float32 expert rows, bf16 output, split 0; seed {args.seed}")
    for model in (m for m in args.models.split(",") if m):
        count, K, k, hidden = SHAPES[model]
        n = k
        gate, up, down = experts_of(count, k, hidden, args.seed)
        staged = packed.PackedMoE(gate, up, down, decode_max_rows=256)
        fused = packed.PackedMoE(gate, up, down, decode_max_rows=256, decode_route="fused")
        gate, up, down = staged.experts.gate, staged.experts.up, staged.experts.down
        g = torch.Generator(device="cuda").manual_seed(args.seed + count)
        for T in (int(v) for v in args.tokens.split(",")):
            S = T * K
            logits = torch.randn((T, count), generator=g, device="cuda")
            top = torch.topk(logits, K, dim=-1)
            ids, w = top.indices.contiguous(), torch.softmax(top.values, dim=-1).float().contiguous()
            x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)
            plan = packed.moe_plan(ids, count, workspace=torch.empty((hb.moe_plan_workspace_bytes(T, K, count),), dtype=torch.uint8, device="cuda"))
            glu_need = hb.packed_glu_skinny_grouped_workspace_bytes(S, count, hidden, k)
            lin_need, down_need = hb.packed_linear_skinny_grouped_workspace_bytes(S, count, n, hidden), hb.moe_down_combine_workspace_bytes(S, count, n, hidden)
            ws = torch.empty((max(glu_need, lin_need, down_need),), dtype=torch.uint8, device="cuda")
            xs = torch.empty((S, k), dtype=torch.bfloat16, device="cuda")
            h_s, h_f = (torch.zeros((S, hidden), dtype=torch.bfloat16, device="cuda") for _ in range(2))
            ys = torch.zeros((S, n), dtype=torch.float32, device="cuda")
            y_s, y_f = (torch.empty((T, n), dtype=torch.bfloat16, device="cuda") for _ in range(2))
            rows, src, row_of = plan.group_rows.data_ptr(), plan.src.data_ptr(), plan.row_of.data_ptr()
            dcall = (x.data_ptr(), T, k, k, src, K, xs.data_ptr(), k, stream)
            gcall = (xs.data_ptr(), S, k, k, rows, *arena_args(gate), *arena_args(up), count, hidden, None, None, 0, silu, h_s.data_ptr(), bf16, hidden, 0,
                     ws.data_ptr(), glu_need, stream)
            fcall = (x.data_ptr(), T, K, k, k, src, rows, *arena_args(gate), *arena_args(up), count, hidden, None, None, 0, silu, h_f.data_ptr(), bf16,
                     hidden, 0, ws.data_ptr(), glu_need, stream)
            lcall = (h_s.data_ptr(), S, hidden, hidden, rows, *arena_args(down), count, n, None, 0, ys.data_ptr(), f32, n, 0,
                     ws.data_ptr() if lin_need else None, lin_need, stream)
            ccall = (ys.data_ptr(), f32, n, row_of, w.data_ptr(), K, None, 0, 0, T, K, n, y_s.data_ptr(), bf16, n, stream)
            ocall = (h_s.data_ptr(), hidden, hidden, rows, *arena_args(down), count, n, f32, row_of, w.data_ptr(), K, None, 0, 0, T, K, y_f.data_ptr(),
                     bf16, n, 0, ws.data_ptr(), down_need, stream)

            def glu_staged(i):
                hb.check(dispatch_fn(*dcall))
                hb.check(glu_fn(*gcall))

            def down_staged(i):
                hb.check(lin_fn(*lcall))
                hb.check(combine_fn(*ccall))

            glu_staged(0)
            hb.check(gather_fn(*fcall))
            down_staged(0)
            hb.check(down_fn(*ocall))
            a, b = fused(x, ids, w), staged(x, ids, w)
            same = (bool(torch.equal(h_s.view(torch.int16), h_f.view(torch.int16))), bool(torch.equal(y_s.view(torch.int16), y_f.view(torch.int16))),
                    bool(torch.equal(a.view(torch.int16), b.view(torch.int16))))
            say(f"## {model}: count={count} K={K} k=n={k} hidden={hidden} T={T} (S={S}): glu split {glu_need // (2 * S * hidden * 4)}, down split "
                f"{down_need // (S * n * 4)}; bits of glu / down / layer {' / '.join('equal' if s else 'DIFFER' for s in same)}")
            label = {"model": model, "count": count, "K": K, "k": k, "hidden": hidden, "T": T}
            for what, ours, theirs, eq in (("glu", lambda i: hb.check(gather_fn(*fcall)), glu_staged, same[0]),
                                           ("down", lambda i: hb.check(down_fn(*ocall)), down_staged, same[1]),
                                           ("layer", lambda i: fused(x, ids, w), lambda i: staged(x, ids, w), same[2])):
                sides = [{"name": "fused", "fn": ours}, {"name": "staged", "fn": theirs}]
                time_sides(sides, args.rounds, args.window_ms)
                say(f"### {what}")
                report({**label, "what": what}, sides, eq)
            del x, xs, ys, h_s, h_f, y_s, y_f, ws
        del staged, fused, gate, up, down
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
