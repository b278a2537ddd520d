"""mtq_packed_matmul (the product with a packed k × n matrix) and the transposed pack / unpack, timed by tools/packed_linear_bench.py's
method: device events after a warm-up, --rounds rounds of a window each, the sides alternated in one process, the C entries called
directly, the weights rotated over --cold-mb of copies.

  matmul  : P (k × n) in {4096 × 4096, 4096 × 14336, 14336 × 4096}, m in {1, 16, 256, 4096}, an all-bfp8, an all-bfp4 and a greedy map.
            Three sides: mtq_packed_matmul on P's stream; mtq_packed_linear (the block kernel) on the n × k stream of Pᵀ under the
            transposed map (the same tile counts, so the same bytes); torch.matmul on the unpacked bf16 P̂.  Before timing, the bit
            contract is checked: mtq_packed_matmul against mtq_packed_linear on the all-bf16 packing of unpack(P̂)ᵀ.
            `matmul/block-min` is the new kernel's median over the block kernel's MINIMUM of the same run; `spread` is the block
            kernel's median over its minimum (the run's own noise).
  pack    : mtq_pack_tiles_transposed / mtq_unpack_tiles_transposed on the stored n × k weight against mtq_pack_tiles /
            mtq_unpack_tiles on the same tensor under the transposed map; bytes moved over time.

  --skinny: mtq_packed_matmul_skinny (the split-K kernel for m <= 32) at split 0, m in {1, 16, 32}, the same shapes and maps.  Four
            sides: the new entry; mtq_packed_matmul (the route before it, the baseline of the gate); mtq_packed_linear_skinny on the
            n × k stream of Pᵀ under the transposed map (the same tiles, the same bytes); torch.matmul on the unpacked bf16 P̂.  The
            workspace is allocated once.  Before timing, the bit contract is checked: the new entry against mtq_packed_linear_skinny
            on the all-bf16 packing of unpack(P̂)ᵀ at split 0.  `gate` is pass when the new kernel's median is below the block side's
            minimum by more than the block side's own minimum-to-median spread; the last line names the largest m at which every
            row passes (packed.AUTO_MATMUL_SKINNY_MAX_M).  --sweep-splits times explicit splits on the first shape and map.

  --wide  : mtq_packed_matmul_wide (the wide-block kernel for m above the decode range), m in {64, 128, 256, 512, 1024, 2048, 4096}, the
            same shapes and maps.  Four sides: the new entry; mtq_packed_matmul (the route before it, the baseline of the gate);
            mtq_packed_linear_wide on the n × k stream of Pᵀ under the transposed map (the same tiles, the same bytes: the kernel the
            new one is expected to equal in time); torch.matmul on the unpacked bf16 P̂.  Before timing, the bit contract is checked:
            the new entry against mtq_packed_matmul.  `gate` is pass when the new kernel's median is below the block side's minimum by
            more than the block side's own minimum-to-median spread; `vs-lw` says whether the new median is above the wide linear's by
            more than that side's spread; the last line names the smallest m from which on every row passes
            (packed.AUTO_MATMUL_WIDE_MIN_M).

  python tools/packed_matmul_bench.py [--rounds 5] [--window-ms 30] [--out profiles/packed_matmul.txt] [--json out.json]
  python tools/packed_matmul_bench.py --skinny [--sweep-splits 1,2,4,8,16,32,64,128] [--out profiles/packed_matmul_skinny.txt]
  python tools/packed_matmul_bench.py --wide [--out profiles/packed_matmul_wide.txt]
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
from tools.packed_linear_bench import calibrate, greedy_map, window_ms


def _calibrate(fn, target_ms: float) -> int:
    """calibrate() with room for a 20 us kernel to fill the window."""
    fn(0)
    torch.cuda.synchronize()
    one = max(window_ms(fn, 20), 1e-4)
    return int(min(max(target_ms / one, 5), 4000))


def _timed(fns, args):
    """(medians, minima) in ms of the sides `fns`, alternated round by round."""
    iters = [_calibrate(fn, args.window_ms) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(args.rounds):
        for j, fn in enumerate(fns):
            ts[j].append(window_ms(fn, iters[j]))
    return [statistics.median(t) for t in ts], [min(t) for t in ts]


def skinny(args, say, rows) -> None:
    if not hb.has_packed_matmul_skinny():
        raise hb.MtqError("this build of libmtq_hip.so lacks mtq_packed_matmul_skinny")
    stream = torch.cuda.current_stream().cuda_stream
    e_new, e_blk, e_lin = hb._entry("mtq_packed_matmul_skinny"), hb._entry("mtq_packed_matmul"), hb._entry("mtq_packed_linear_skinny")
    ms = [int(v) for v in args.ms.split(",")]
    passed = {m: True for m in ms}
    first = True
    for shape in args.shapes.split(","):
        k, n = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + k)
        pm = (torch.randn((k, n), generator=g, device="cuda") * 0.02).to(torch.bfloat16)      # P, k × n
        w = pm.t().contiguous()
        th, tw = hb.tiles_hw(k, n)
        maps = {"bfp8": lambda: np.full((th, tw), 1, dtype=np.int8), "bfp4": lambda: np.full((th, tw), 2, dtype=np.int8), "greedy": lambda: greedy_map(pm)}
        need = hb.packed_matmul_skinny_workspace_bytes(32, n, k, 0)
        for s in args.sweep_splits:
            need = max(need, hb.packed_matmul_skinny_workspace_bytes(32, n, k, s))
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")                  # once, for every m and split
        for name in args.maps.split(","):
            amap = maps[name]()
            counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
            tp = hb.PackedTables.on_device(amap)                                              # over P's grid
            tl = hb.PackedTables.on_device(np.ascontiguousarray(amap.T))                      # over W's grid: the same counts
            dp = hb.pack_tiles(pm, tp)
            dl = hb.pack_tiles(w, tl)
            pq = hb.unpack_tiles(dp, tp, k, n, dtype=torch.bfloat16)                          # P̂ bf16, k × n
            tb = hb.PackedTables.on_device(np.zeros(hb.tiles_hw(n, k), dtype=np.int8))
            db = hb.pack_tiles(pq.t().contiguous(), tb)                                       # the contract pair
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / tp.nbytes)))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (2 * n * k))))
            dps = [dp] + [dp.clone() for _ in range(copies_p - 1)]
            dls = [dl] + [dl.clone() for _ in range(copies_p - 1)]
            pqs = [pq] + [pq.clone() for _ in range(copies_w - 1)]
            for m in ms:
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                ya, yb, yc, ym = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(4))

                def equal_bits(split):
                    hb.packed_matmul_skinny(x, dp, tp, n, out_dtype=torch.bfloat16, out=ya, split=split, workspace=ws)   # the wrappers' checks, once
                    hb.packed_linear_skinny(x, db, tb, n, out_dtype=torch.bfloat16, out=yb, split=split, workspace=ws)
                    return bool(torch.equal(ya.view(torch.int16), yb.view(torch.int16)))

                same = equal_bits(0)

                def new_calls(split):
                    return [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tp.nbytes, tp.map_ptr, tp.offsets_ptr, n, None, ya.data_ptr(), hb.DTYPE_BF16, n,
                             split, ws.data_ptr(), ws.numel(), stream) for d in dps]

                c_new = new_calls(0)
                c_blk = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tp.nbytes, tp.map_ptr, tp.offsets_ptr, n, None, yc.data_ptr(), hb.DTYPE_BF16, n,
                          stream) for d in dps]
                c_lin = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tl.nbytes, tl.map_ptr, tl.offsets_ptr, n, None, yb.data_ptr(), hb.DTYPE_BF16, n,
                          0, ws.data_ptr(), ws.numel(), stream) for d in dls]

                def f_new(i):
                    hb.check(e_new(*c_new[i % copies_p]))

                def f_blk(i):
                    hb.check(e_blk(*c_blk[i % copies_p]))

                def f_lin(i):
                    hb.check(e_lin(*c_lin[i % copies_p]))

                def f_torch(i):
                    torch.matmul(x, pqs[i % copies_w], out=ym)

                med, mn = _timed((f_new, f_blk, f_lin, f_torch), args)
                f_new(0)
                f_torch(0)
                err = float((ya.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                gate = med[0] < mn[1] - (med[1] - mn[1])
                passed[m] = passed[m] and gate and same
                rows.append({"what": "packed_matmul_skinny", "k": k, "n": n, "m": m, "map": name, "counts": counts, "skinny_ms_median": med[0],
                             "skinny_ms_min": mn[0], "block_ms_median": med[1], "block_ms_min": mn[1], "linear_skinny_ms_median": med[2],
                             "linear_skinny_ms_min": mn[2], "torch_ms_median": med[3], "torch_ms_min": mn[3], "skinny_over_block_min": med[0] / mn[1],
                             "block_spread": med[1] / mn[1], "skinny_over_linear_skinny": med[0] / med[2], "skinny_over_torch": med[0] / med[3],
                             "stream_gbs": tp.nbytes / med[0] / 1e6, "gate": bool(gate), "contract_bits_equal": same, "max_rel_diff_torch": err})
                say(f"skinny P {k}x{n} m={m:3d} map={name:6s} new {med[0] * 1e3:7.1f} us (min {mn[0] * 1e3:7.1f}, {tp.nbytes / med[0] / 1e6:7.1f} GB/s of stream) "
                    f"block {med[1] * 1e3:7.1f} us (min {mn[1] * 1e3:7.1f}) linear-skinny {med[2] * 1e3:7.1f} us (min {mn[2] * 1e3:7.1f}) "
                    f"torch {med[3] * 1e3:7.1f} us (min {mn[3] * 1e3:7.1f})  new/block-min {med[0] / mn[1]:6.3f} spread {med[1] / mn[1]:5.3f} "
                    f"gate {'pass' if gate else 'FAIL'}  new/linear-skinny {med[0] / med[2]:5.2f} new/torch {med[0] / med[3]:5.2f}  "
                    f"contract bits equal: {same}  max rel diff to torch {err:.2e}")
                if first and args.sweep_splits:          # explicit splits on the first shape and map, the linear skinny kernel beside it
                    for split in args.sweep_splits:
                        ok = equal_bits(split)
                        c_s = new_calls(split)
                        c_l = [c[:13] + (split,) + c[14:] for c in c_lin]
                        med_s, mn_s = _timed((lambda i: hb.check(e_new(*c_s[i % copies_p])), lambda i: hb.check(e_lin(*c_l[i % copies_p]))), args)
                        rows.append({"what": "packed_matmul_skinny_split", "k": k, "n": n, "m": m, "map": name, "split": split, "skinny_ms_median": med_s[0],
                                     "skinny_ms_min": mn_s[0], "linear_skinny_ms_median": med_s[1], "linear_skinny_ms_min": mn_s[1], "contract_bits_equal": ok})
                        say(f"  split sweep P {k}x{n} m={m:3d} map={name:6s} split={split:4d} new {med_s[0] * 1e3:7.1f} us (min {mn_s[0] * 1e3:7.1f}) "
                            f"linear-skinny {med_s[1] * 1e3:7.1f} us (min {mn_s[1] * 1e3:7.1f})  contract bits equal: {ok}")
            first = False
            del dps, dls, pqs, dp, dl, pq, db
        del pm, w, ws
    good = [m for m in ms if passed[m]]
    say(f"# gate: every shape and map passes at m in {good}; AUTO_MATMUL_SKINNY_MAX_M = {max(good) if good else None}")


def wide(args, say, rows) -> None:
    if not hb.has_packed_matmul_wide():
        raise hb.MtqError("this build of libmtq_hip.so lacks mtq_packed_matmul_wide")
    stream = torch.cuda.current_stream().cuda_stream
    e_new, e_blk, e_lw = hb._entry("mtq_packed_matmul_wide"), hb._entry("mtq_packed_matmul"), hb._entry("mtq_packed_linear_wide")
    ms = sorted(int(v) for v in args.ms.split(","))
    passed = {m: True for m in ms}
    worst = None                                             # the row whose new median is furthest above the wide linear's
    for shape in args.shapes.split(","):
        k, n = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + k)
        pm = (torch.randn((k, n), generator=g, device="cuda") * 0.02).to(torch.bfloat16)      # P, k × n
        w = pm.t().contiguous()
        th, tw = hb.tiles_hw(k, n)
        maps = {"bfp8": lambda: np.full((th, tw), 1, dtype=np.int8), "bfp4": lambda: np.full((th, tw), 2, dtype=np.int8), "greedy": lambda: greedy_map(pm)}
        for name in args.maps.split(","):
            amap = maps[name]()
            counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
            tp = hb.PackedTables.on_device(amap)                                              # over P's grid
            tl = hb.PackedTables.on_device(np.ascontiguousarray(amap.T))                      # over W's grid: the same counts
            assert tp.nbytes == tl.nbytes
            dp = hb.pack_tiles(pm, tp)
            dl = hb.pack_tiles(w, tl)
            pq = hb.unpack_tiles(dp, tp, k, n, dtype=torch.bfloat16)                          # P̂ bf16, k × n
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / tp.nbytes)))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (2 * n * k))))
            dps = [dp] + [dp.clone() for _ in range(copies_p - 1)]
            dls = [dl] + [dl.clone() for _ in range(copies_p - 1)]
            pqs = [pq] + [pq.clone() for _ in range(copies_w - 1)]
            for m in ms:
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                ya, yb, yc, ym = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(4))
                hb.packed_matmul_wide(x, dp, tp, n, out_dtype=torch.bfloat16, out=ya)          # the wrappers' checks, once
                hb.packed_matmul(x, dp, tp, n, out_dtype=torch.bfloat16, out=yc)
                same = bool(torch.equal(ya.view(torch.int16), yc.view(torch.int16)))
                c_new = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tp.nbytes, tp.map_ptr, tp.offsets_ptr, n, None, ya.data_ptr(), hb.DTYPE_BF16, n,
                          stream) for d in dps]
                c_blk = [c[:10] + (yc.data_ptr(),) + c[11:] for c in c_new]
                c_lw = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tl.nbytes, tl.map_ptr, tl.offsets_ptr, n, None, yb.data_ptr(), hb.DTYPE_BF16, n,
                         stream) for d in dls]

                def f_new(i):
                    hb.check(e_new(*c_new[i % copies_p]))

                def f_blk(i):
                    hb.check(e_blk(*c_blk[i % copies_p]))

                def f_lw(i):
                    hb.check(e_lw(*c_lw[i % copies_p]))

                def f_torch(i):
                    torch.matmul(x, pqs[i % copies_w], out=ym)

                med, mn = _timed((f_new, f_blk, f_lw, f_torch), args)
                f_new(0)
                f_torch(0)
                err = float((ya.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                gate = med[0] < mn[1] - (med[1] - mn[1])
                above = med[0] > med[2] + (med[2] - mn[2])                                    # above the wide linear by more than its spread
                passed[m] = passed[m] and gate and same
                if above and (worst is None or med[0] / med[2] > worst[0]):
                    worst = (med[0] / med[2], f"P {k}x{n} m={m} map={name}")
                flop = 2.0 * m * n * k
                rows.append({"what": "packed_matmul_wide", "k": k, "n": n, "m": m, "map": name, "counts": counts, "wide_ms_median": med[0],
                             "wide_ms_min": mn[0], "block_ms_median": med[1], "block_ms_min": mn[1], "linear_wide_ms_median": med[2],
                             "linear_wide_ms_min": mn[2], "torch_ms_median": med[3], "torch_ms_min": mn[3], "wide_over_block_min": med[0] / mn[1],
                             "block_spread": med[1] / mn[1], "wide_over_linear_wide": med[0] / med[2], "linear_wide_spread": med[2] / mn[2],
                             "above_linear_wide": bool(above), "wide_over_torch": med[0] / med[3], "wide_tflops": flop / med[0] / 1e9,
                             "gate": bool(gate), "contract_bits_equal": same, "max_rel_diff_torch": err})
                say(f"wide P {k}x{n} m={m:4d} map={name:6s} new {med[0] * 1e3:8.1f} us (min {mn[0] * 1e3:8.1f}, {flop / med[0] / 1e9:6.1f} TFLOP/s) "
                    f"block {med[1] * 1e3:8.1f} us (min {mn[1] * 1e3:8.1f}) linear-wide {med[2] * 1e3:8.1f} us (min {mn[2] * 1e3:8.1f}) "
                    f"torch {med[3] * 1e3:8.1f} us (min {mn[3] * 1e3:8.1f})  new/block-min {med[0] / mn[1]:6.3f} spread {med[1] / mn[1]:5.3f} "
                    f"gate {'pass' if gate else 'FAIL'}  new/linear-wide {med[0] / med[2]:5.3f} its spread {med[2] / mn[2]:5.3f} "
                    f"vs-lw {'ABOVE' if above else 'within'}  new/torch {med[0] / med[3]:5.2f}  bits equal the block kernel's: {same}  "
                    f"max rel diff to torch {err:.2e}")
            del dps, dls, pqs, dp, dl, pq
        del pm, w
    from_m = None                                            # the smallest m from which on every measured m passes
    for m in reversed(ms):
        if not passed[m]:
            break
        from_m = m
    say(f"# gate: every shape and map passes at m in {[m for m in ms if passed[m]]}; AUTO_MATMUL_WIDE_MIN_M = {from_m}")
    say(f"# rows whose median is above the wide linear's by more than that side's spread: "
        f"{'none' if worst is None else 'worst ' + worst[1] + f' at {worst[0]:.3f}'}")


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=30.0)
    p.add_argument("--cold-mb", type=float, default=640.0, help="rotate over copies of the weight worth this many MB")
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--shapes", default="4096x4096,4096x14336,14336x4096", help="k x n of the packed matrix, comma separated")
    p.add_argument("--ms", default="1,16,256,4096")
    p.add_argument("--maps", default="bfp8,bfp4,greedy")
    p.add_argument("--skip-pack", action="store_true", help="skip the pack / unpack timings")
    p.add_argument("--skinny", action="store_true", help="time mtq_packed_matmul_skinny (m <= 32) against the block entry, the skinny linear and torch")
    p.add_argument("--wide", action="store_true", help="time mtq_packed_matmul_wide (m >= 64) against the block entry, the wide linear and torch")
    p.add_argument("--sweep-splits", default="", help="--skinny: explicit splits timed on the first shape and map, comma separated")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    if not hb.has_packed_matmul():
        raise hb.MtqError("this build of libmtq_hip.so lacks mtq_packed_matmul")
    rows, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    if args.wide:
        args.ms = "64,128,256,512,1024,2048,4096" if args.ms == p.get_default("ms") else args.ms
        say(f"# mtq_packed_matmul_wide on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
            f"sides alternated, weights rotated over {args.cold_mb:.0f} MB, bf16 output")
        wide(args, say, rows)
        return finish(args, lines, rows)
    if args.skinny:
        args.ms = "1,16,32" if args.ms == p.get_default("ms") else args.ms
        args.sweep_splits = [int(v) for v in args.sweep_splits.split(",") if v]
        say(f"# mtq_packed_matmul_skinny on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
            f"sides alternated, weights rotated over {args.cold_mb:.0f} MB, bf16 output, split 0 unless named")
        skinny(args, say, rows)
        return finish(args, lines, rows)
    say(f"# mtq_packed_matmul on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, "
        f"weights rotated over {args.cold_mb:.0f} MB; HBM figure {args.hbm_tbs} TB/s")
    stream = torch.cuda.current_stream().cuda_stream
    for shape in args.shapes.split(","):
        k, n = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + k)
        pm = (torch.randn((k, n), generator=g, device="cuda") * 0.02).to(torch.bfloat16)      # P, k × n
        w = pm.t().contiguous()                                                               # W = Pᵀ, n × k as a linear layer stores it
        th, tw = hb.tiles_hw(k, n)
        maps = {"bfp8": lambda: np.full((th, tw), 1, dtype=np.int8), "bfp4": lambda: np.full((th, tw), 2, dtype=np.int8), "greedy": lambda: greedy_map(pm)}
        for name in args.maps.split(","):
            amap = maps[name]()
            counts = np.bincount(amap.reshape(-1), minlength=4).tolist()
            tp = hb.PackedTables.on_device(amap)                                              # over P's grid
            tl = hb.PackedTables.on_device(np.ascontiguousarray(amap.T))                      # over W's grid: the same counts
            assert tp.nbytes == tl.nbytes
            dp = hb.pack_tiles_transposed(w, tp)                                              # P's stream, from W read in place
            assert torch.equal(dp, hb.pack_tiles(pm, tp))
            dl = hb.pack_tiles(w, tl)                                                         # W's row-layout stream: the block kernel's side
            pq = hb.unpack_tiles(dp, tp, k, n, dtype=torch.bfloat16)                          # P̂ bf16, k × n
            if not args.skip_pack:
                y16 = torch.empty((n, k), dtype=torch.bfloat16, device="cuda")
                sides = (("pack_transposed", lambda i: hb.pack_tiles_transposed(w, tp, out=dp), 2 * n * k + tp.nbytes),
                         ("pack_rows", lambda i: hb.pack_tiles(w, tl, out=dl), 2 * n * k + tl.nbytes),
                         ("unpack_transposed_bf16", lambda i: hb.unpack_tiles_transposed(dp, tp, n, k, dtype=torch.bfloat16, out=y16), tp.nbytes + 2 * n * k),
                         ("unpack_rows_bf16", lambda i: hb.unpack_tiles(dl, tl, n, k, dtype=torch.bfloat16, out=y16), tl.nbytes + 2 * n * k))
                iters = [calibrate(fn, args.window_ms) for _w, fn, _b in sides]
                ts = [[] for _ in sides]
                for _ in range(args.rounds):
                    for j, (_w, fn, _b) in enumerate(sides):
                        ts[j].append(window_ms(fn, iters[j]))
                for j, (what, _fn, moved) in enumerate(sides):
                    med = statistics.median(ts[j])
                    rows.append({"what": what, "n": n, "k": k, "map": name, "counts": counts, "ms_median": med, "ms_min": min(ts[j]), "bytes": moved,
                                 "tbs": moved / med / 1e9})
                    say(f"{what:22s} W {n}x{k} map={name:6s} counts={counts} {med * 1e3:9.1f} us (min {min(ts[j]) * 1e3:9.1f})  "
                        f"{moved / med / 1e9:6.3f} TB/s = {100 * moved / med / 1e9 / args.hbm_tbs:5.1f}% of {args.hbm_tbs} TB/s")
                del y16
            # the contract pair: the all-bf16 row-layout packing of unpack(P̂)ᵀ
            tb = hb.PackedTables.on_device(np.zeros(hb.tiles_hw(n, k), dtype=np.int8))
            db = hb.pack_tiles(pq.t().contiguous(), tb)
            copies_p = max(2, int(np.ceil(args.cold_mb * 1e6 / tp.nbytes)))
            copies_w = max(2, int(np.ceil(args.cold_mb * 1e6 / (2 * n * k))))
            dps = [dp] + [dp.clone() for _ in range(copies_p - 1)]
            dls = [dl] + [dl.clone() for _ in range(copies_p - 1)]
            pqs = [pq] + [pq.clone() for _ in range(copies_w - 1)]
            for m in (int(v) for v in args.ms.split(",")):
                x = torch.randn((m, k), generator=g, device="cuda").to(torch.bfloat16)
                ya, yb, ym = (torch.empty((m, n), dtype=torch.bfloat16, device="cuda") for _ in range(3))
                hb.packed_matmul(x, dp, tp, n, out_dtype=torch.bfloat16, out=ya)               # the wrappers' checks, once
                hb.packed_linear(x, db, tb, n, out_dtype=torch.bfloat16, out=yb)
                same = bool(torch.equal(ya.view(torch.int16), yb.view(torch.int16)))
                e_mm, e_lin = hb._entry("mtq_packed_matmul"), hb._entry("mtq_packed_linear")
                c_mm = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tp.nbytes, tp.map_ptr, tp.offsets_ptr, n, None, ya.data_ptr(), hb.DTYPE_BF16, n,
                         stream) for d in dps]
                c_lin = [(x.data_ptr(), m, k, x.stride(0), d.data_ptr(), tl.nbytes, tl.map_ptr, tl.offsets_ptr, n, None, yb.data_ptr(), hb.DTYPE_BF16, n,
                          stream) for d in dls]

                def f_mm(i):
                    hb.check(e_mm(*c_mm[i % copies_p]))

                def f_lin(i):
                    hb.check(e_lin(*c_lin[i % copies_p]))

                def f_torch(i):
                    torch.matmul(x, pqs[i % copies_w], out=ym)

                fns = (f_mm, f_lin, f_torch)
                iters = [calibrate(fn, args.window_ms) for fn in fns]
                ts = [[], [], []]
                for _ in range(args.rounds):
                    for j, fn in enumerate(fns):
                        ts[j].append(window_ms(fn, iters[j]))
                f_mm(0)
                f_torch(0)
                err = float((ya.float() - ym.float()).abs().max() / ym.float().abs().max().clamp_min(1e-30))
                med = [statistics.median(t) for t in ts]
                mn = [min(t) for t in ts]
                flop = 2.0 * m * n * k
                rows.append({"what": "packed_matmul", "k": k, "n": n, "m": m, "map": name, "counts": counts, "matmul_ms_median": med[0],
                             "matmul_ms_min": mn[0], "block_ms_median": med[1], "block_ms_min": mn[1], "torch_ms_median": med[2], "torch_ms_min": mn[2],
                             "matmul_over_block_min": med[0] / mn[1], "block_spread": med[1] / mn[1], "matmul_over_torch": med[0] / med[2],
                             "stream_gbs": tp.nbytes / med[0] / 1e6, "matmul_tflops": flop / med[0] / 1e9, "block_tflops": flop / med[1] / 1e9,
                             "torch_tflops": flop / med[2] / 1e9, "contract_bits_equal": same, "max_rel_diff_torch": err})
                say(f"matmul P {k}x{n} m={m:5d} map={name:6s} new {med[0] * 1e3:9.1f} us (min {mn[0] * 1e3:9.1f}, {tp.nbytes / med[0] / 1e6:7.1f} GB/s of stream) "
                    f"block {med[1] * 1e3:9.1f} us (min {mn[1] * 1e3:9.1f}) torch {med[2] * 1e3:9.1f} us (min {mn[2] * 1e3:9.1f})  "
                    f"matmul/block-min {med[0] / mn[1]:6.3f} spread {med[1] / mn[1]:5.3f} matmul/torch {med[0] / med[2]:6.2f}  "
                    f"contract bits equal: {same}  max rel diff to torch {err:.2e}")
            del dps, dls, pqs, dp, dl, pq, db
        del pm, w
    return finish(args, lines, rows)


def finish(args, lines, rows) -> int:
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
