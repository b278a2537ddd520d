"""mixed-tile-budget on one MI355X: the device allocator, the batched table launch and BudgetPipeline against what there was before them.

  (a) allocate : mtq_budget_allocate_device (device events around the whole call: hull, the bisection passes, the final map) against
                 budget_maps.allocate on the same table brought to the host — per segment, the table's copy home included, as a caller
                 without the device allocator pays it.  Tables are real: the e_w of Gaussian bf16 weights with outlier columns, at
                 T = 16 384 (one 4096² tensor) as 1 segment and as 128 segments of 128 tiles, and at the tile count of the
                 synthetic:llama3-8b selection as one segment (the first table tiled with a per-tile scale of e^U(-3, 3)).  Before any
                 timing the device maps and counts are compared with the host's.
  (b) table    : mtq_tile_sq_error_batched over --tensors x --n² bf16 in one launch against the loop of mtq_tile_error_tables calls with
                 zero Gram blocks (the only route to e_w before), device events; GB/s = input bytes / time.
  (c) pipeline : BudgetPipeline.run against ThresholdPipeline.run (pcc 0.999) on the same resident batch, wall clock to a synchronise,
                 alternated, for scale: the two answer different questions.

  python tools/budget_bench.py [--tensors 128] [--n 4096] [--rounds 7] [--out profiles/budget_allocate.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.model_source import build_model_index, resolve_selected_tensors
from quantization_analysis_amd.pipeline import BudgetPipeline, ThresholdPipeline

ALL = list(hb.MIXED_TILE_FORMATS)
BITS = 4.5


def event_ms(fn, reps: int) -> list:
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def fmt(v) -> str:
    return f"{statistics.median(v):10.3f} [{min(v):10.3f}]"


def llama_tiles() -> int:
    index = build_model_index("synthetic:llama3-8b")
    total = 0
    for name in resolve_selected_tensors(index, None):
        shape, _dtype = index.shape_dtype(name)
        rows, cols = (-(-int(shape[0]) // 32), 32) if len(shape) == 1 else (int(np.prod(shape[:-1])), int(shape[-1]))
        total += -(-rows // 32) * -(-cols // 32)
    return total


def allocator_row(name: str, table, first: np.ndarray, rounds: int, host_rounds: int) -> tuple:
    T, n_seg = int(table.shape[0]), len(first) - 1
    budgets = [BITS / 8.0 * 1024.0 * float(n) for n in np.diff(first)]
    first_dev = torch.from_numpy(first).cuda()
    budget_dev = torch.tensor(budgets, dtype=torch.float64, device="cuda")
    scratch = torch.empty((hb.budget_allocate_scratch_bytes(T, n_seg),), dtype=torch.uint8, device="cuda")

    def device():
        return hb.budget_allocate_device(table, first_dev, ALL, budget_dev, scratch)

    def host():
        t = table.cpu().numpy()
        return [bm.allocate(t[a:b], ALL, BITS) for a, b in zip(first[:-1], first[1:])]

    maps, counts, status = device()
    want = host()
    same = bool((status == 0).all()) and all(np.array_equal(maps[a:b].cpu().numpy(), w[0].reshape(-1)) and counts[j].tolist() == [w[1][f] for f in ALL]
                                             for j, (a, b, w) in enumerate(zip(first[:-1], first[1:], want)))
    dev_ms = event_ms(device, rounds + 2)[2:]
    host_ms = []
    for _ in range(host_rounds):
        t0 = time.perf_counter()
        host()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    ratio = statistics.median(host_ms) / statistics.median(dev_ms)
    line = f"  {name:34s} device {fmt(dev_ms)}   host {fmt(host_ms)}   host / device {ratio:8.1f}x   equal maps and counts: {same}"
    return ("**" + line.strip() + "**" if ratio < 1.0 else line), same


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--tensors", type=int, default=128)
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--big-host-rounds", type=int, default=2)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.rounds < 5:
        p.error("--rounds must be at least 5 (medians of fewer say little)")

    hb.require_gpu()   # no device, no numbers
    count, n = args.tensors, args.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((count, n, n), generator=gen, device="cuda", dtype=torch.float32) * 0.02
    x[:, :, ::61] *= 12.0                                           # outlier columns: tiles of different sensitivity
    x = x.to(torch.bfloat16)
    th, tw = hb.tiles_hw(n, n)
    tiles = th * tw
    lines = [f"budget_bench: {count} x {n}x{n} bf16 ({x.numel() * 2 / 2**30:.2f} GiB resident), {tiles} tiles per tensor, {BITS} bits, "
             f"{torch.cuda.get_device_name(0)}, rounds {args.rounds}",
             "times in ms, medians, minima in brackets; a row in bold is one the device loses"]
    ok = True

    # (b) first: its table feeds (a)
    h0 = torch.zeros((tw, 32, 32), dtype=torch.float64, device="cuda")
    batched = hb.tile_sq_error_batched(x)
    looped = torch.stack([hb.tile_error_tables(x[i], h0, want_weight=True)[1] for i in range(count)])
    same = torch.equal(batched.view(torch.int64), looped.view(torch.int64))
    ok = ok and same
    out = torch.empty_like(batched)
    k_b = event_ms(lambda: hb.tile_sq_error_batched(x, out=out), args.rounds + 2)[2:]
    k_l = event_ms(lambda: [hb.tile_error_tables(x[i], h0, want_weight=True) for i in range(count)], args.rounds + 2)[2:]
    gb = x.numel() * 2 / 1e9
    ratio = statistics.median(k_l) / statistics.median(k_b)
    lines += ["", f"(b) e_w of {count} tensors; batched and looped tables bit-identical: {same}",
              f"  mtq_tile_sq_error_batched, one launch      {fmt(k_b)}  {gb / statistics.median(k_b) * 1e3:8.1f} GB/s",
              f"  loop of mtq_tile_error_tables, zero H     {fmt(k_l)}  {gb / statistics.median(k_l) * 1e3:8.1f} GB/s",
              ("**" if ratio < 1.0 else "") + f"  loop / batched: {ratio:.2f}x" + ("**" if ratio < 1.0 else "")]
    del looped, out

    # (a)
    lines += ["", "(a) allocation at 4.5 bits, device call against budget_maps.allocate on the table brought home"]
    one = batched[0].contiguous()
    row, same = allocator_row(f"T = {tiles}, 1 segment", one, np.array([0, tiles], dtype=np.int64), args.rounds, args.rounds)
    lines.append(row)
    ok = ok and same
    row, same = allocator_row(f"T = {tiles}, 128 segments", one, np.arange(0, tiles + 1, tiles // 128, dtype=np.int64), args.rounds, args.rounds)
    lines.append(row)
    ok = ok and same
    big = llama_tiles()
    g = torch.Generator(device="cuda").manual_seed(2)
    scale = torch.exp(torch.rand((big, 1), generator=g, device="cuda", dtype=torch.float64) * 6.0 - 3.0)
    table = one[torch.arange(big, device="cuda") % tiles] * scale
    row, same = allocator_row(f"T = {big} (llama3-8b), 1 segment", table, np.array([0, big], dtype=np.int64), args.rounds, args.big_host_rounds)
    lines.append(row)
    ok = ok and same
    del table, scale, batched

    # (c)
    with BudgetPipeline(ALL, "pcc", BITS, chunk=1 << 30) as bp, ThresholdPipeline(ALL, "pcc", 0.999, chunk=1 << 30) as tp:
        sides = {"BudgetPipeline.run": lambda: bp.run(x), "ThresholdPipeline.run": lambda: tp.run(x)}
        for fn in sides.values():
            wall_ms(fn)
        wall = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                wall[name].append(wall_ms(fn))
    lines += ["", f"(c) one batch of {count} x {n}² through a pipeline, wall clock to a synchronise (results on the host)"]
    for name in sides:
        lines.append(f"  {name:28s}{fmt(wall[name])}")
    ratio = statistics.median(wall["ThresholdPipeline.run"]) / statistics.median(wall["BudgetPipeline.run"])
    lines.append(("**" if ratio < 1.0 else "") + f"  threshold / budget: {ratio:.2f}x" + ("**" if ratio < 1.0 else ""))
    if not ok:
        lines.append("MISMATCH: a timing above compares different results")

    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
