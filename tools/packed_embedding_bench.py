"""The packed input embedding (csrc/mtq_packed_gather.hip, mtq_packed_embedding), timed with device events after a warm-up.

  Tables 128256 x 4096 and 129280 x 7168 (bf16), tokens in {1, 32, 512, 4096}, an all-bfp8 map and a mixed map (seeded: half bfp8, three
  tenths bfp4, a tenth each bf16 and bfp2), the stream of the table ("rows") and of its transpose ("transpose").  Three sides alternated
  in the same process, --rounds rounds of a window each, median and minimum per call:
      packed    the C entry into a preallocated bf16 output (at 1 token the binding's Python checks would be what is timed);
      torch     torch.nn.functional.embedding on the unpacked bf16 table, which has to stay resident for it;
      unpack+   unpack of the whole table to bf16, then an index: what packed.py offered before the kernel.
  Each side rotates over --id-sets sets of uniformly drawn int64 ids.  The line states the resident bytes of both forms of the table and
  the output bytes over the packed kernel's time (the bytes a gather has to write; the stream bytes it reads are at most as many).
  No ratio is required of the kernel: the capability is the deliverable, the numbers are the record.

  python tools/packed_embedding_bench.py [--rounds 5] [--window-ms 20] [--out profiles/packed_embedding.txt] [--json out.json]
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


def window_ms(fn, iters: int) -> float:
    """Milliseconds per call of `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def calibrate(fn, target_ms: float) -> int:
    fn(0)
    torch.cuda.synchronize()
    one = max(window_ms(fn, 3), 1e-3)
    return int(min(max(target_ms / one, 3), 400))


def maps_of(grid) -> dict:
    mixed = np.random.default_rng(123).choice(np.array([0, 1, 2, 3], dtype=np.int8), size=grid, p=[0.1, 0.5, 0.3, 0.1])
    return {"bfp8": np.full(grid, 1, dtype=np.int8), "mixed": mixed}


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--shapes", default="128256x4096,129280x7168")
    p.add_argument("--tokens", default="1,32,512,4096")
    p.add_argument("--id-sets", type=int, default=8)
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    rows, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# packed embedding on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"{args.id_sets} id sets per side")
    entry, stream = hb._entry("mtq_packed_embedding"), torch.cuda.current_stream().cuda_stream
    for shape in args.shapes.split(","):
        vocab, hidden = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(vocab + hidden)
        w = (torch.randn((vocab, hidden), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        for stored in ("rows", "transpose"):
            srows, scols = (hidden, vocab) if stored == "transpose" else (vocab, hidden)
            for name, amap in maps_of(hb.tiles_hw(srows, scols)).items():
                tables = hb.PackedTables.on_device(amap)
                if stored == "transpose":
                    data = hb.pack_tiles_transposed(w, tables)
                    table = hb.unpack_tiles_transposed(data, tables, vocab, hidden, dtype=torch.bfloat16)
                    unpack = lambda: hb.unpack_tiles_transposed(data, tables, vocab, hidden, dtype=torch.bfloat16, out=table)   # noqa: E731
                else:
                    data = hb.pack_tiles(w, tables)
                    table = hb.unpack_tiles(data, tables, vocab, hidden, dtype=torch.bfloat16)
                    unpack = lambda: hb.unpack_tiles(data, tables, vocab, hidden, dtype=torch.bfloat16, out=table)   # noqa: E731
                counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
                packed_resident = tables.nbytes + amap.size + 4 * (amap.size + 1)
                for tokens in (int(v) for v in args.tokens.split(",")):
                    idsets = [torch.randint(0, vocab, (tokens,), generator=g, device="cuda") for _ in range(args.id_sets)]
                    y = torch.empty((tokens, hidden), dtype=torch.bfloat16, device="cuda")
                    got = hb.packed_embedding(idsets[0], data, tables, srows, scols, stored=int(stored == "transpose"), out=y)   # the checks, once
                    same = bool(torch.equal(got.view(torch.int16), table[idsets[0]].view(torch.int16)))
                    calls = [(i.data_ptr(), hb.IDS_I64, tokens, 0, data.data_ptr(), tables.nbytes, tables.map_ptr, tables.offsets_ptr, srows, scols,
                              int(stored == "transpose"), 0, 0.0, y.data_ptr(), hb.DTYPE_BF16, hidden, stream) for i in idsets]
                    sides = {"packed": lambda i: hb.check(entry(*calls[i % args.id_sets])),
                             "torch": lambda i: torch.nn.functional.embedding(idsets[i % args.id_sets], table),
                             "unpack+": lambda i: unpack()[idsets[i % args.id_sets]]}
                    iters = {k: calibrate(fn, args.window_ms) for k, fn in sides.items()}
                    ts = {k: [] for k in sides}
                    for _ in range(args.rounds):
                        for k, fn in sides.items():
                            ts[k].append(window_ms(fn, iters[k]))
                    med = {k: statistics.median(v) for k, v in ts.items()}
                    out_bytes = tokens * hidden * 2
                    rows.append({"vocab": vocab, "hidden": hidden, "stored": stored, "map": name, "counts": counts, "tokens": tokens,
                                 "packed_resident_bytes": packed_resident, "bf16_resident_bytes": 2 * vocab * hidden, "bits_equal_table": same,
                                 **{f"{k}_ms_median": med[k] for k in sides}, **{f"{k}_ms_min": min(ts[k]) for k in sides},
                                 "packed_output_gbs": out_bytes / med["packed"] / 1e6})
                    say(f"{vocab}x{hidden} {stored:9s} map={name:5s} tokens={tokens:5d}  packed {med['packed'] * 1e3:8.1f} us (min {min(ts['packed']) * 1e3:8.1f}, "
                        f"{out_bytes / med['packed'] / 1e6:7.1f} GB/s of output)  torch {med['torch'] * 1e3:8.1f} us (min {min(ts['torch']) * 1e3:8.1f})  "
                        f"unpack+index {med['unpack+'] * 1e3:9.1f} us  packed/torch {med['packed'] / med['torch']:6.2f}  "
                        f"resident {packed_resident / 1e6:7.1f} MB packed, {2 * vocab * hidden / 1e6:7.1f} MB bf16  bits equal table: {same}")
                del data, table, tables
        del w
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
