"""packed.pack_batch_transposed against the loop of packed.pack_transposed it replaces, and against packed.pack_batch of the same bytes in
the row layout, on batches resident on the device: --groups (a llama3-8b layer's k / v group, 2 x 1024x4096, and one large group,
32 x 4096x4096) in bf16 and float32 storage, under a uniform bfp4 map and a random map of 85 % bfp8 / 15 % bfp4 tiles (the greedy map's
mix).  The large group is 1 GiB (bf16) or 2 GiB (float32) in: past the 256 MiB Infinity Cache, an HBM figure; the small
group (16 / 32 MB) is served from the cache after the warm-up.

  kernels : device events around each call, --reps calls after a warm-up, tables already on the device:
              mtq_pack_tiles_transposed_batched (the staged read, or the direct read in a library built with
              -DMTQ_PACK_TRANSPOSED_BATCHED_DIRECT and given as MTQ_LIB: the A/B of the read path), mtq_pack_tiles_batched on the same
              bytes (the row read, a yardstick), and mtq_pack_tiles_transposed on each matrix in turn (a window of back-to-back launches
              between two events, per batch).  GB/s = (input bytes + arena bytes) over the time.
  routes  : wall clock from the call to a device synchronise, alternated in one process after a warm-up of each, --rounds rounds:
              (a) packed.pack_batch_transposed(w, maps)
              (b) [packed.pack_transposed(w[i], maps[i]) for i]: a map upload, a host offsets pass and a launch per tensor
              (c) packed.pack_batch(w, row maps with the same codes): the same number of bytes read by rows
  Before any timing the arena of (a) is compared with the streams of (b) byte for byte.

  python tools/pack_batch_transposed_bench.py [--groups 2x1024x4096,32x4096x4096] [--rounds 7] [--reps 20] [--out FILE] [--json FILE]
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
from tools.pack_batch_bench import event_ms, wall_ms, window_ms


def maps_of(kind: str, count: int, tiles_h: int, tiles_w: int) -> np.ndarray:
    if kind == "bfp4":
        return np.full((count, tiles_h, tiles_w), 2, dtype=np.int8)
    rng = np.random.default_rng(85)
    return np.where(rng.random((count, tiles_h, tiles_w)) < 0.85, 1, 2).astype(np.int8)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--groups", default="2x1024x4096,32x4096x4096", help="comma-separated COUNTxNxK batches of (n, k) weights")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    if args.rounds < 5:
        p.error("--rounds must be at least 5 (medians of fewer say little)")
    groups = [tuple(int(v) for v in g.split("x")) for g in args.groups.split(",")]

    hb.require_gpu()   # no device, no numbers
    if not hb.has_packed_batch_transposed():
        raise SystemExit(f"{hb.LIB_PATH} lacks the batched transposed entries")
    lines = [f"pack_batch_transposed_bench: {torch.cuda.get_device_name(0)}, library {hb.LIB_PATH.name}, rounds {args.rounds}, reps {args.reps}",
             "times in ms, medians with minima in brackets; GB/s = (input + arena bytes) / median time"]
    record = {"library": str(hb.LIB_PATH.name), "rounds": args.rounds, "reps": args.reps, "cases": []}
    ok = True

    def med(v):
        return statistics.median(v)

    def row(label, v, moved):
        return f"  {label:58s}{med(v):9.3f} [{min(v):9.3f}]  {moved / med(v) / 1e6:8.1f} GB/s"

    for count, n, k in groups:
        th, tw = hb.tiles_hw(k, n)                                # the transposes' grid
        tiles = th * tw
        for storage in (torch.bfloat16, torch.float32):
            gen = torch.Generator(device="cuda").manual_seed(1)
            w = (torch.randn((count, n, k), generator=gen, device="cuda", dtype=torch.float32) * 0.02).to(storage)
            in_bytes = w.numel() * w.element_size()
            for kind in ("bfp4", "85/15"):
                maps = maps_of(kind, count, th, tw)
                row_maps = np.ascontiguousarray(maps.transpose(0, 2, 1))          # W's own grid, the same codes: the same arena length

                def loop():
                    return [packed.pack_transposed(w[i], maps[i], backend="hip") for i in range(count)]

                pts = packed.pack_batch_transposed(w, maps, backend="hip")
                batch = packed.batch_of(pts)
                singles = loop()
                same = all(torch.equal(a.data, b.data) for a, b in zip(pts, singles))
                ok = ok and same
                rows_pts = packed.pack_batch(w, row_maps, backend="hip")
                rows_batch = packed.batch_of(rows_pts)
                arena_bytes = batch.arena.numel()
                assert rows_batch.arena.numel() == arena_bytes
                moved = in_bytes + arena_bytes
                del singles

                out = torch.empty_like(batch.arena)
                k_t = event_ms(lambda: hb.pack_tiles_transposed_batched(w, batch.maps_dev, batch.offsets_dev, batch.bases_dev, out), args.reps + 3)[3:]
                k_r = event_ms(lambda: hb.pack_tiles_batched(w, rows_batch.maps_dev, rows_batch.offsets_dev, rows_batch.bases_dev, out), args.reps + 3)[3:]
                tables = [pt.tables() for pt in pts]

                def each_in_turn():
                    for i in range(count):
                        hb.pack_tiles_transposed(w[i], tables[i], out=pts[i].data)

                each_in_turn()
                k_one = [window_ms(each_in_turn, max(1, 64 // count)) for _ in range(args.rounds)]      # per walk over the batch
                del out

                sides = {"(a) pack_batch_transposed": lambda: packed.pack_batch_transposed(w, maps, backend="hip"),
                         "(b) loop of pack_transposed": loop,
                         "(c) pack_batch, row layout, the same bytes": lambda: packed.pack_batch(w, row_maps, backend="hip")}
                for fn in sides.values():
                    wall_ms(fn)
                wall = {name: [] for name in sides}
                for _ in range(args.rounds):
                    for name, fn in sides.items():
                        wall[name].append(wall_ms(fn))

                name = f"{count} x {n}x{k} {'bf16' if storage == torch.bfloat16 else 'f32'}, map {kind}"
                lines.append("")
                lines.append(f"{name}: input {in_bytes / 1e9:.3f} GB, arena {arena_bytes / 1e9:.3f} GB; batched and looped streams byte-identical: {same}")
                lines.append(row("kernel mtq_pack_tiles_transposed_batched", k_t, moved))
                lines.append(row("kernel mtq_pack_tiles_batched (row read)", k_r, moved))
                lines.append(row(f"kernel mtq_pack_tiles_transposed, {count} launches in turn", k_one, moved))
                for side in sides:
                    lines.append(row(side, wall[side], moved))
                a, b = wall["(a) pack_batch_transposed"], wall["(b) loop of pack_transposed"]
                lines.append(f"  (b) / (a): {med(b) / med(a):.2f}x by medians, {min(b) / min(a):.2f}x by minima")
                record["cases"].append({"case": name, "same_bytes": bool(same), "input_bytes": in_bytes, "arena_bytes": arena_bytes,
                                        "kernel_transposed_batched_ms": k_t, "kernel_row_batched_ms": k_r, "kernel_transposed_in_turn_ms": k_one,
                                        "wall_ms": wall})
                if not same:
                    lines.append("  MISMATCH: the timings above compare different results")
                del pts, batch, rows_pts, rows_batch, tables
            del w

    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(record) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
