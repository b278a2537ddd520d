#!/usr/bin/env python3
"""Layer-output error of quantised weights on recorded activations (the consumer of the files the reference's
scripts/generate_deepseek_layer0_io.py writes).  For every selected op: R = X·Wᵀ (+ b) against Y_f = X·Ŵ_fᵀ (+ b) for each format
and for the map of the compression config's mixed-tile algorithm, as pcc / mae / atol over all outputs, plus a `recorded` row
(R against the recorded output).  --x-format bfp8 / bfp4 / bfp2 feeds every candidate BFP-quantised activations Q(X) (R keeps X).  Weights come from quantization_analysis_amd.model_source (synthetic presets or a local safetensors
directory); io_root is a directory in the reference's layout or `synthetic:<tokens>[:seed]`.  --budget-bits B ... adds, per B, the
maps budget:<B>:output and budget:<B>:weight chosen on the calibration activations (--calib-io / --calib-split, quantization_analysis_amd
/budget_maps.py) and evaluated like every other candidate.  --gptq adds GPTQ error-compensated weights built on the same calibration
activations (quantization_analysis_amd/gptq.py): gptq:<bfp*>, gptq:<map> and gptq:budget:<B>:output, each at its RTN counterpart's bytes.
--transpose (implied by a config with the transpose algorithm) adds <bfp*>+transpose, Ŵ = quantize(Wᵀ)ᵀ with one shared exponent per 16
rows of a column, and with --budget-bits the maps budget:<B>:<basis>+transpose over Wᵀ's grid; a mixed-tile config with
"layout": "transpose" gives map:<algorithm>+transpose.  GPTQ stays row-layout only unless --gptq-transpose (with --gptq and --transpose)
is given: the transposed candidates are then swept in the transposed layout, on the same Hessian and factor, as gptq:<bfp*>+transpose,
gptq:<map> of a transposed map and gptq:budget:<B>:output+transpose, each at its +transpose RTN counterpart's bytes.

  python scripts/layer_output_error.py /path/to/DeepSeek-R1 /path/to/io model.layers.0.mlp --backend hip -c bf16 bfp8 bfp4 bfp2 \\
      --compression-config compression_configs/compression_config.mixed_tile_greedy.example.json --split test --out-dir results/loe
"""
from __future__ import annotations

import argparse
import csv
import math
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np

from quantization_analysis_amd.budget_maps import bits_tag
from quantization_analysis_amd.compression_algorithms import load_compression_config
from quantization_analysis_amd.hadamard import check_block
from quantization_analysis_amd.layer_io import select_ops
from quantization_analysis_amd.model_source import build_model_index, resolve_format_list
from quantization_analysis_amd.output_error import BACKENDS, LAYOUTS, X_FORMATS, check_layout, evaluate_op
from quantization_analysis_amd.quantization_formats import BASE_FORMATS as SUPPORTED_FORMATS  # no proxy rows here


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Layer-output error of quantised weights on recorded activations.")
    p.add_argument("repo_or_url", help="'synthetic:<preset>[:seed]' or a local directory of *.safetensors.")
    p.add_argument("io_root", help="Directory of recorded op inputs / outputs (reference layout) or 'synthetic:<tokens>[:seed]'.")
    p.add_argument("filter_query", nargs="*", help="Optional filter on the op weights: substring, or dotted torch-style prefix path.")
    p.add_argument("--revision", default="main")
    p.add_argument("--backend", choices=list(BACKENDS), default="emulation", help="emulation = float64 on the host; hip = MI355X kernel.")
    p.add_argument("-c", "--formats", nargs="+", default=None, help="Candidate formats (default: the config's, else all).")
    p.add_argument("--compression-config", default=None, help="A mixed-tile config adds the map of its search as a candidate.")
    p.add_argument("--split", choices=["calibration", "test", "all"], default="all")
    p.add_argument("--max-samples", type=int, default=None, help="First N samples of the split (by sample index).")
    p.add_argument("--chunk-rows", type=int, default=16384, help="Activation rows per kernel launch (partial sums are carried).")
    p.add_argument("--x-format", choices=list(X_FORMATS), default="bf16",
                   help="Activation format the candidates see: bf16 = X as recorded; bfp* = Q(X) in the row layout (R keeps X).")
    p.add_argument("--out-dir", default="results/layer_output_error")
    p.add_argument("--budget-bits", type=float, nargs="+", default=None, metavar="B",
                   help="Bits per weight: each adds the maps budget:<B>:output (activation-aware) and budget:<B>:weight (weight-only).")
    p.add_argument("--calib-io", default=None, help="Calibration activations of the budget maps (default: io_root).")
    p.add_argument("--calib-split", choices=["calibration", "test", "all"], default="calibration")
    p.add_argument("--calib-max-samples", type=int, default=None, help="First N calibration samples (by sample index).")
    p.add_argument("--save-maps", action="store_true",
                   help="Write <out-dir>/maps/<op>/budget_<B>_{output,weight}.npy (and budget_<B>_<basis>_transpose.npy over Wᵀ's grid).")
    p.add_argument("--transpose", action="store_true",
                   help="Add the transposed BFP layout: <bfp*>+transpose and, with --budget-bits, budget:<B>:<basis>+transpose.")
    p.add_argument("--gptq", action="store_true",
                   help="Add GPTQ error-compensated weights built on the calibration activations: gptq:<bfp*>, gptq:<map>, gptq:budget:<B>:output.")
    p.add_argument("--gptq-damp", type=float, default=0.01, metavar="D", help="GPTQ damping: λ = D · mean(diag H) (finite, > 0).")
    p.add_argument("--gptq-factor", choices=("host", "device"), default="host",
                   help="Where GPTQ factorises the damped Hessian: host (CPU LAPACK) or device (the hip backend's float64 MFMA kernels).")
    p.add_argument("--gptq-transpose", action="store_true",
                   help="With --gptq and --transpose: GPTQ rows of the transposed candidates too, swept in the transposed layout "
                        "(gptq:<bfp*>+transpose, gptq:<map> of a transposed map, gptq:budget:<B>:output+transpose).")
    p.add_argument("--rotate", default=None, metavar="{B|auto}",
                   help="Evaluate every op rotated by a block Hadamard transform along k: B a power of two in [32, 4096], or auto = the "
                        "largest one dividing k.  An op whose k the block does not divide is skipped.")
    p.add_argument("--awq", action="store_true",
                   help="Add AWQ rows: per-input-channel power-of-two scales searched on the calibration activations, awq:<bfp*> and awq:<map>.")
    p.add_argument("--awq-grid", type=int, default=20, metavar="G", help="AWQ: values of α tried, α = g / G for g = 0 .. G − 1.")
    p.add_argument("--awq-max-shift", type=int, default=7, metavar="P", help="AWQ: the largest exponent shift, 1 .. 7.")
    args = p.parse_args(argv)
    if args.awq:
        if args.x_format != "bf16":
            p.error("--awq needs --x-format bf16: the shifts are searched and evaluated on bf16 activations")
        if args.awq_grid < 1 or not 1 <= args.awq_max_shift <= 7:
            p.error("--awq-grid must be >= 1 and --awq-max-shift in 1 .. 7")
    if args.rotate is not None and args.rotate != "auto":
        try:
            args.rotate = check_block(int(args.rotate), int(args.rotate))
        except ValueError as e:
            p.error(f"--rotate: {e}")
    if args.gptq_transpose and not (args.gptq and args.transpose):
        p.error("--gptq-transpose needs --gptq and --transpose: it adds the GPTQ rows of the transposed candidates")
    if args.gptq:
        if args.x_format != "bf16":
            p.error("--gptq needs --x-format bf16: the GPTQ weights are built and evaluated on bf16 activations")
    if args.gptq_factor == "device" and args.backend != "hip":
        p.error("--gptq-factor device needs --backend hip: the emulation factorises on the host")
    if not (math.isfinite(args.gptq_damp) and args.gptq_damp > 0.0):
        p.error(f"--gptq-damp: {args.gptq_damp:g} is not finite and > 0")
    if args.budget_bits:
        if args.x_format != "bf16":
            p.error("--budget-bits needs --x-format bf16: the budget maps are chosen and evaluated on bf16 activations")
        for b in args.budget_bits:
            if not 0.0 < b <= 16.0:
                p.error(f"--budget-bits: {b:g} is outside (0, 16]")
    return args


def _fmt(v, spec):
    return "-" if v is None else format(v, spec)


def main(argv=None) -> int:
    args = parse_args(argv)
    config = load_compression_config(args.compression_config) if args.compression_config else None
    check_layout(config, LAYOUTS)
    transpose = args.transpose or (config is not None and config.algorithm == "transpose")
    formats = resolve_format_list(args.formats or (config.quantization_formats if config else None), SUPPORTED_FORMATS)
    if args.backend == "hip":
        import torch

        torch.cuda.set_device(0)
    index = build_model_index(args.repo_or_url, revision=args.revision)
    query = " ".join(args.filter_query).strip() or None
    ops, skipped = select_ops(index, args.io_root, query, args.split, args.max_samples)
    budgets = tuple(args.budget_bits or ())
    calib_io = args.calib_io or args.io_root
    calib = {}
    if budgets or args.gptq or args.awq:
        cal_ops, _cal_skipped = select_ops(index, calib_io, query, args.calib_split, args.calib_max_samples)
        calib = {o.op: o for o in cal_ops}
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    records, csv_rows = [], []
    for op in ops:
        extra = {"budgets": budgets, "calib": calib.get(op.op)} if budgets or args.gptq or args.awq else {}
        if args.gptq:
            extra.update(gptq=True, gptq_damp=args.gptq_damp, gptq_factor=args.gptq_factor)
        if args.gptq_transpose:
            extra.update(gptq_transpose=True)
        if args.awq:
            extra.update(awq=True, awq_grid=args.awq_grid, awq_max_shift=args.awq_max_shift)
        if transpose:
            extra.update(transpose=True)
        if args.rotate:
            extra.update(rotate=args.rotate)
        res = evaluate_op(index, op, formats, config, args.backend, args.chunk_rows, args.x_format, **extra)
        if res.skipped:
            skipped.append((op.op, res.skipped))
            continue
        n, k = res.shape
        xf = f"  X {res.x_format}" if res.x_format != "bf16" else ""
        xf += f"  rotated by H_{res.rotate}" if res.rotate else ""
        print(f"\n{res.op}  W {n}x{k}{xf}  M {res.m}  splits {','.join(res.splits)}{'  (X cast to bf16)' if res.x_cast else ''}")
        print(f"{'candidate':<28} | {'bytes':>14} | {'pcc':>12} | {'mae':>12} | {'atol':>12}")
        print("-" * 90)
        for r in res.rows:
            print(f"{r.candidate:<28} | {_fmt(r.bytes, '14.0f')} | {r.pcc:12.8f} | {r.mae:12.6e} | {r.atol:12.6e}")
            csv_rows.append([res.op, r.candidate, r.bytes, r.pcc, r.mae, r.atol, res.m, n, k] + ([res.rotate] if args.rotate else [])
                            + ([r.extra.get("alpha"), r.extra.get("calib_loss") if "alpha" in r.extra else None] if args.awq else []))
        rec = {"op": res.op, "weight": res.weight, "shape": [n, k], "M": res.m, "splits": res.splits, "x_cast": res.x_cast,
               "rows": [{"candidate": r.candidate, "bytes": r.bytes, "pcc": r.pcc, "mae": r.mae, "atol": r.atol,
                         **{key: v for key, v in r.extra.items() if key not in ("assignment", "exponents")}} for r in res.rows]}
        if args.rotate:
            rec["rotate"] = res.rotate
        if budgets or args.gptq or args.awq:
            rec["calib_splits"] = res.calib_splits
            rec["budget_skipped"] = [{"candidate": c, "reason": why} for c, why in res.budget_skipped]
            for c, why in res.budget_skipped:
                skipped.append((f"{res.op} {c}", why))
            if args.save_maps:
                for r in res.rows:
                    if "assignment" in r.extra:
                        d = out_dir / "maps" / res.op
                        d.mkdir(parents=True, exist_ok=True)
                        tag = "_transpose" if r.extra.get("layout") == "transpose" else ""
                        np.save(d / f"budget_{bits_tag(r.extra['bits'])}_{r.extra['basis']}{tag}.npy", r.extra["assignment"])
                    if "exponents" in r.extra:
                        d = out_dir / "maps" / res.op
                        d.mkdir(parents=True, exist_ok=True)
                        np.save(d / f"{r.candidate.replace(':', '_')}_exponents.npy", r.extra["exponents"])
        records.append(rec)
    if skipped:
        print("\nskipped:")
        for op, why in skipped:
            print(f"  {op}: {why}")
    with open(out_dir / "layer_output_error.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["op", "candidate", "bytes", "pcc", "mae", "atol", "M", "N", "K"] + (["rotate"] if args.rotate else [])
                   + (["awq_alpha", "awq_calib_loss"] if args.awq else []))
        w.writerows(csv_rows)
    doc = {"repo_or_url": args.repo_or_url, "io_root": args.io_root, "backend": args.backend, "formats": formats,
           "compression_config": args.compression_config, "split": args.split, "max_samples": args.max_samples, "x_format": args.x_format,
           "ops": records, "skipped": [{"op": o, "reason": r} for o, r in skipped]}
    if budgets:
        doc.update({"budget_bits": list(budgets)})
    if budgets or args.gptq or args.awq:
        doc.update({"calib_io": calib_io, "calib_split": args.calib_split, "calib_max_samples": args.calib_max_samples})
    if args.gptq:
        doc.update({"gptq_damp": args.gptq_damp, "gptq_factor": args.gptq_factor})
    if args.gptq_transpose:
        doc.update({"gptq_transpose": True})
    if args.awq:
        doc.update({"awq_grid": args.awq_grid, "awq_max_shift": args.awq_max_shift})
    if transpose:
        doc.update({"transpose": True})
    if args.rotate:
        doc.update({"rotate": args.rotate})
    (out_dir / "layer_output_error.json").write_text(json.dumps(doc, indent=2))
    print(f"\nwrote {out_dir / 'layer_output_error.csv'} and {out_dir / 'layer_output_error.json'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
