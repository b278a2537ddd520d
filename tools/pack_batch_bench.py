"""packed.pack_batch against the loop of packed.pack it replaces, on a batch the size of a search pipeline's: --tensors (128) matrices of
--n × --n (4096²) bf16, resident on the device (4 GiB in, 1.2–2.3 GB out: far past the 256 MiB Infinity Cache, so every figure here
is an HBM figure), under a uniform bfp8 map, a uniform bfp4 map and a random map of 85 % bfp8 / 15 % bfp4 tiles (the greedy map's mix,
DESIGN.md §A.6g).

  (a) kernels : the batched pack kernel alone (mtq_pack_tiles_batched, tables already on the device) and the batched offsets kernels
                alone, device events around each call, the median of --reps calls after a warm-up.  TB/s = (input bytes + arena bytes)
                over the kernel's time.  Beside it the single-tensor kernel (mtq_pack_tiles, ~25 µs: windows of 200 / 2 x tensors
                back-to-back calls between two events, per call) on ONE matrix of the batch again and again (32 MB in: the Infinity
                Cache regime §A.6g measured) and on each matrix of the batch in turn (the HBM regime; launches included in both).
  (b) pack_batch : wall clock of packed.pack_batch from the call to a device synchronise, with host maps and with device maps.
  (c) the loop   : wall clock of [packed.pack(x[i], maps[i], backend="hip") for i in range(tensors)] and a synchronise: the route there
                was before pack_batch, the baseline.
  (b) and (c) alternate in one process after a warm-up of each; medians (and minima) of --rounds rounds.  Before any timing the arena of
  (b) is compared with the streams of (c) byte for byte.

  python tools/pack_batch_bench.py [--tensors 128] [--n 4096] [--rounds 7] [--reps 20] [--out profiles/pack_batch.txt] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed


def event_ms(fn, reps: int) -> list:
    """Milliseconds of each of `reps` calls, a pair of device events around every call."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def window_ms(fn, iters: int) -> float:
    """Milliseconds per call of `iters` back-to-back calls between two device events (for calls too short for a pair of events each)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def maps_of(kind: str, count: int, tiles_h: int, tiles_w: int) -> np.ndarray:
    if kind == "bfp8":
        return np.full((count, tiles_h, tiles_w), 1, dtype=np.int8)
    if kind == "bfp4":
        return np.full((count, tiles_h, tiles_w), 2, dtype=np.int8)
    rng = np.random.default_rng(85)
    return np.where(rng.random((count, tiles_h, tiles_w)) < 0.85, 1, 2).astype(np.int8)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--tensors", type=int, default=128)
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    if args.rounds < 5:
        p.error("--rounds must be at least 5 (medians of fewer say little)")

    hb.require_gpu()   # no device, no numbers
    count, n = args.tensors, args.n
    th, tw = hb.tiles_hw(n, n)
    tiles = th * tw
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((count, n, n), generator=gen, device="cuda", dtype=torch.float32) * 0.02).to(torch.bfloat16)
    in_bytes = x.numel() * 2
    lines = [f"pack_batch_bench: {count} x {n}x{n} bf16 ({in_bytes / 2**30:.2f} GiB resident), {tiles} tiles per tensor, "
             f"{torch.cuda.get_device_name(0)}, rounds {args.rounds}, reps {args.reps}",
             "times in ms; TB/s = (input + arena bytes) / kernel time; medians, minima in brackets"]
    record = {"tensors": count, "n": n, "rounds": args.rounds, "reps": args.reps, "maps": {}}

    def med(v):
        return statistics.median(v)

    for kind in ("bfp8", "bfp4", "85/15"):
        maps = maps_of(kind, count, th, tw)
        maps_dev = torch.from_numpy(maps.reshape(count, tiles)).cuda()

        def loop():
            return [packed.pack(x[i], maps[i], backend="hip") for i in range(count)]

        # the same bytes first
        pts = packed.pack_batch(x, maps, backend="hip")
        batch = packed.batch_of(pts)
        singles = loop()
        same = all(torch.equal(a.data, b.data) for a, b in zip(pts, singles))
        same = same and torch.equal(packed.batch_of(packed.pack_batch(x, maps_dev.reshape(count, th, tw), backend="hip")).arena, batch.arena)
        arena_bytes = batch.arena.numel()
        moved = in_bytes + arena_bytes
        del singles

        # (a) kernels alone
        out = torch.empty_like(batch.arena)
        k_pack = event_ms(lambda: hb.pack_tiles_batched(x, batch.maps_dev, batch.offsets_dev, batch.bases_dev, out), args.reps + 3)[3:]
        k_offs = event_ms(lambda: hb.packed_offsets_device(maps_dev, count, tiles), args.reps + 3)[3:]
        one_tables = pts[0].tables()
        one_out = torch.empty((one_tables.nbytes,), dtype=torch.uint8, device="cuda")
        one = lambda: hb.pack_tiles(x[0], one_tables, out=one_out)   # noqa: E731
        window_ms(one, 20)
        k_one_cached = [window_ms(one, 200) for _ in range(args.rounds)]
        tables = [pt.tables() for pt in pts]
        state = {"i": 0}

        def one_in_turn():
            i = state["i"] = (state["i"] + 1) % count
            hb.pack_tiles(x[i], tables[i], out=pts[i].data)

        window_ms(one_in_turn, count)
        k_one_hbm = [window_ms(one_in_turn, 2 * count) for _ in range(args.rounds)]
        one_moved = n * n * 2 + one_tables.nbytes
        del out

        # (b) and (c), alternated
        sides = {"pack_batch, host maps": lambda: packed.pack_batch(x, maps, backend="hip"),
                 "pack_batch, device maps": lambda: packed.pack_batch(x, maps_dev.reshape(count, th, tw), backend="hip"),
                 "loop of pack": loop}
        for fn in sides.values():
            wall_ms(fn)
        wall = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                wall[name].append(wall_ms(fn))

        lines.append("")
        lines.append(f"map {kind}: arena {arena_bytes / 1e9:.3f} GB; batched and looped streams byte-identical: {same}")
        lines.append(f"  (a) pack_tiles_batched kernel   {med(k_pack):8.3f} [{min(k_pack):8.3f}]  {moved / med(k_pack) / 1e9:6.2f} TB/s")
        lines.append(f"      offsets + bases kernels     {med(k_offs):8.3f} [{min(k_offs):8.3f}]  (includes three device allocations)")
        lines.append(f"      pack_tiles, one matrix again and again (Infinity Cache) {med(k_one_cached):7.4f} [{min(k_one_cached):7.4f}]  {one_moved / med(k_one_cached) / 1e9:6.2f} TB/s")
        lines.append(f"      pack_tiles, each matrix in turn (HBM)                   {med(k_one_hbm):7.4f} [{min(k_one_hbm):7.4f}]  {one_moved / med(k_one_hbm) / 1e9:6.2f} TB/s")
        for name in sides:
            lines.append(f"  {'(c)' if name == 'loop of pack' else '(b)'} {name:28s}{med(wall[name]):8.2f} [{min(wall[name]):8.2f}]")
        base = med(wall["loop of pack"])
        lines.append(f"      loop / pack_batch: {base / med(wall['pack_batch, host maps']):.2f}x (host maps), {base / med(wall['pack_batch, device maps']):.2f}x (device maps)")
        record["maps"][kind] = {"same_bytes": bool(same), "arena_bytes": arena_bytes, "kernel_pack_ms": k_pack, "kernel_offsets_ms": k_offs,
                                "kernel_single_cached_ms": k_one_cached, "kernel_single_hbm_ms": k_one_hbm, "wall_ms": wall}
        del pts, batch, tables
        if not same:
            lines.append("  MISMATCH: the timings above compare different results")

    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(record) + "\n")
    return 0 if all(m["same_bytes"] for m in record["maps"].values()) else 1


if __name__ == "__main__":
    raise SystemExit(main())
