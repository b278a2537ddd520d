"""The activation prologue of a rotated / AWQ-scaled packed layer at decode sizes: inside the skinny kernel (prologue="fused",
mtq_packed_linear_skinny_pre / mtq_packed_glu_skinny_pre) against the staged route (hadamard, torch.ldexp, then the skinny product), by
the method of DESIGN.md §A.6g: the outputs compared first, device events after a warm-up, the sides alternated in one process, --rounds
rounds of a window each, medians.

Module rows: PackedLinear(kernel="skinny") at n x k in --shapes, m in --ms, block in --blocks, with and without shifts, all-bfp4 maps:
  floor    the unrotated module (no prologue), the time the product alone takes;
  staged   prologue="staged", today's route; timed TWICE per round (staged, staged2): the spread between the two medians is what a
           difference has to exceed to count;
  fused    prologue="fused".
PackedMLP(decode_kernel="fused") at --mlp (k x hidden), rotate = down_rotate = the first block, staged and fused.
Kernel rows (`k` in front of the shape): the same three sides through the hip_backend entries with prebuilt outputs and workspaces, no
module around them - hadamard_rows, torch.ldexp and packed_linear_skinny against packed_linear_skinny_pre, at the first shape.
--staged-only times floor and staged alone: run on a build of the parent commit (where PackedLinear has no prologue argument) it gives
the parent's staged leg for the same rows.

  python tools/packed_prologue_bench.py [--rounds 5] [--window-ms 20] [--out profiles/packed_prologue.txt]
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
from tools.packed_linear_bench import calibrate, window_ms


def time_sides(sides, rounds: int, target_ms: float) -> None:
    for s in sides:
        s["iters"], s["ts"] = calibrate(s["fn"], target_ms), []
    for _ in range(rounds):
        for s in sides:                              # alternated: every side sees every phase of the clocks
            s["ts"].append(window_ms(s["fn"], s["iters"]) * 1e3)
    for s in sides:
        s["med"] = statistics.median(s["ts"])


def packed_weight(n: int, k: int, seed: int):
    w = torch.randn((n, k), generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()
    return packed.pack(w, np.full((-(-n // 32), k // 32), 2, dtype=np.int8), backend="hip")


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    p.add_argument("--ms", default="1,8,32")
    p.add_argument("--blocks", default="32,256,1024")
    p.add_argument("--mlp", default="4096x14336")
    p.add_argument("--staged-only", action="store_true")
    p.add_argument("--out", default="profiles/packed_prologue.txt")
    a = p.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    blocks, ms = [int(b) for b in a.blocks.split(",")], [int(m) for m in a.ms.split(",")]
    lines = [f"# tools/packed_prologue_bench.py --rounds {a.rounds} --window-ms {a.window_ms}{' --staged-only' if a.staged_only else ''}: "
             "medians in us per forward; all-bfp4 maps; PackedLinear(kernel='skinny', out bf16)",
             f"{'n x k':>13} {'m':>3} {'block':>5} {'shifts':>6} {'floor':>8} {'staged':>8} {'staged2':>8} {'fused':>8} {'fused/staged':>12} {'spread':>7}"]
    extra = {} if a.staged_only else {"prologue": "fused"}
    for shape in a.shapes.split(","):
        n, k = (int(v) for v in shape.split("x"))
        pt = packed_weight(n, k, n + k)
        floor = packed.PackedLinear(pt, kernel="skinny", out_dtype="bfloat16")
        for B in blocks:
            for shifts in (None, rng.integers(0, 8, k)):
                staged = packed.PackedLinear(pt, kernel="skinny", out_dtype="bfloat16", rotate=B, in_exponents=shifts)
                fused = None if a.staged_only else packed.PackedLinear(pt, kernel="skinny", out_dtype="bfloat16", rotate=B, in_exponents=shifts, **extra)
                for m in ms:
                    x = torch.randn((m, k), device="cuda").to(torch.bfloat16)
                    sides = [{"name": "floor", "fn": lambda i, f=floor, x=x: f(x)}, {"name": "staged", "fn": lambda i, f=staged, x=x: f(x)},
                             {"name": "staged2", "fn": lambda i, f=staged, x=x: f(x)}]
                    if fused is not None:
                        got, want = fused(x).float(), staged(x).float()          # equal splits give equal bits; the rules may differ
                        err = float((got - want).abs().max() / want.abs().max())
                        assert err < 2e-2, (shape, B, m, err)
                        sides.append({"name": "fused", "fn": lambda i, f=fused, x=x: f(x)})
                    time_sides(sides, a.rounds, a.window_ms)
                    t = {s["name"]: s["med"] for s in sides}
                    fu = t.get("fused")
                    lines.append(f"{shape:>13} {m:>3} {B:>5} {'yes' if shifts is not None else 'no':>6} {t['floor']:>8.1f} {t['staged']:>8.1f} "
                                 f"{t['staged2']:>8.1f} " + (f"{fu:>8.1f} {fu / min(t['staged'], t['staged2']):>12.3f}" if fu else f"{'-':>8} {'-':>12}")
                                 + f" {abs(t['staged'] - t['staged2']):>7.2f}")
                    print(lines[-1], flush=True)
    n, k = (int(v) for v in a.shapes.split(",")[0].split("x"))
    pt = packed_weight(n, k, n + k)
    data, tables = packed._device_data(pt), pt.tables()
    for B in blocks:
        for shifts in (None, torch.from_numpy(rng.integers(0, 8, k).astype(np.uint8)).cuda()):
            neg = None if shifts is None else -shifts.to(torch.int32)
            for m in ms:
                x, xr = torch.randn((m, k), device="cuda").to(torch.bfloat16), torch.empty((m, k), device="cuda", dtype=torch.bfloat16)
                y, ws = torch.empty((m, n), device="cuda", dtype=torch.bfloat16), torch.empty((hb.packed_linear_skinny_workspace_bytes(m, n, k),), dtype=torch.uint8, device="cuda")

                def staged(i):
                    hb.hadamard_rows(x, B, out=xr)
                    hb.packed_linear_skinny(xr if neg is None else torch.ldexp(xr, neg), data, tables, n, out_dtype=torch.bfloat16, out=y, workspace=ws)

                sides = [{"name": "floor", "fn": lambda i: hb.packed_linear_skinny(x, data, tables, n, out_dtype=torch.bfloat16, out=y, workspace=ws)},
                         {"name": "staged", "fn": staged}, {"name": "staged2", "fn": staged}]
                if not a.staged_only:
                    sides.append({"name": "fused", "fn": lambda i: hb.packed_linear_skinny_pre(x, data, tables, n, block=B, in_exponents=shifts,
                                                                                               out_dtype=torch.bfloat16, out=y, workspace=ws)})
                time_sides(sides, a.rounds, a.window_ms)
                t = {s["name"]: s["med"] for s in sides}
                fu = t.get("fused")
                lines.append(f"{'k ' + a.shapes.split(',')[0]:>13} {m:>3} {B:>5} {'yes' if shifts is not None else 'no':>6} {t['floor']:>8.1f} {t['staged']:>8.1f} "
                             f"{t['staged2']:>8.1f} " + (f"{fu:>8.1f} {fu / min(t['staged'], t['staged2']):>12.3f}" if fu else f"{'-':>8} {'-':>12}")
                             + f" {abs(t['staged'] - t['staged2']):>7.2f}")
                print(lines[-1], flush=True)
    k, hidden = (int(v) for v in a.mlp.split("x"))
    gate, up, down = packed_weight(hidden, k, 1), packed_weight(hidden, k, 2), packed_weight(k, hidden, 3)
    lines.append(f"# PackedMLP {k} -> {hidden} -> {k}, decode_kernel='fused', rotate = down_rotate = {blocks[0]}, shifts on x")
    kw = dict(decode_kernel="fused", rotate=blocks[0], down_rotate=blocks[0], in_exponents=rng.integers(0, 8, k)) if not a.staged_only else None
    for m in ms:
        x = torch.randn((m, k), device="cuda").to(torch.bfloat16)
        sides = [{"name": "floor", "fn": lambda i, f=packed.PackedMLP(gate, up, down, decode_kernel="fused"), x=x: f(x)}]
        if kw:
            for name in ("staged", "staged2", "fused"):
                mod = packed.PackedMLP(gate, up, down, prologue=name.rstrip("2"), **kw)
                sides.append({"name": name, "fn": lambda i, f=mod, x=x: f(x)})
        time_sides(sides, a.rounds, a.window_ms)
        lines.append(f"{'mlp':>13} {m:>3} " + " ".join(f"{s['name']} {s['med']:.1f}" for s in sides))
        print(lines[-1], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
