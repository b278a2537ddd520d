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
"layout": "transpose" gives map:<algorithm>+transpose.  GPTQ stays row-layout only.

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
    args = p.parse_args(argv)
    if args.gptq:
        if args.x_format != "bf16":
            p.error("--gptq needs --x-format bf16: the GPTQ weights are built and evaluated on bf16 activations")
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
    if budgets or args.gptq:
        cal_ops, _cal_skipped = select_ops(index, calib_io, query, args.calib_split, args.calib_max_samples)
        calib = {o.op: o for o in cal_ops}
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    records, csv_rows = [], []
    for op in ops:
        extra = {"budgets": budgets, "calib": calib.get(op.op)} if budgets or args.gptq else {}
        if args.gptq:
            extra.update(gptq=True, gptq_damp=args.gptq_damp)
        if transpose:
            extra.update(transpose=True)
        res = evaluate_op(index, op, formats, config, args.backend, args.chunk_rows, args.x_format, **extra)
        if res.skipped:
            skipped.append((op.op, res.skipped))
            continue
        n, k = res.shape
        xf = f"  X {res.x_format}" if res.x_format != "bf16" else ""
        print(f"\n{res.op}  W {n}x{k}{xf}  M {res.m}  splits {','.join(res.splits)}{'  (X cast to bf16)' if res.x_cast else ''}")
        print(f"{'candidate':<28} | {'bytes':>14} | {'pcc':>12} | {'mae':>12} | {'atol':>12}")
        print("-" * 90)
        for r in res.rows:
            print(f"{r.candidate:<28} | {_fmt(r.bytes, '14.0f')} | {r.pcc:12.8f} | {r.mae:12.6e} | {r.atol:12.6e}")
            csv_rows.append([res.op, r.candidate, r.bytes, r.pcc, r.mae, r.atol, res.m, n, k])
        rec = {"op": res.op, "weight": res.weight, "shape": [n, k], "M": res.m, "splits": res.splits, "x_cast": res.x_cast,
               "rows": [{"candidate": r.candidate, "bytes": r.bytes, "pcc": r.pcc, "mae": r.mae, "atol": r.atol,
                         **{key: v for key, v in r.extra.items() if key != "assignment"}} for r in res.rows]}
        if budgets or args.gptq:
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
        records.append(rec)
    if skipped:
        print("\nskipped:")
        for op, why in skipped:
            print(f"  {op}: {why}")
    with open(out_dir / "layer_output_error.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["op", "candidate", "bytes", "pcc", "mae", "atol", "M", "N", "K"])
        w.writerows(csv_rows)
    doc = {"repo_or_url": args.repo_or_url, "io_root": args.io_root, "backend": args.backend, "formats": formats,
           "compression_config": args.compression_config, "split": args.split, "max_samples": args.max_samples, "x_format": args.x_format,
           "ops": records, "skipped": [{"op": o, "reason": r} for o, r in skipped]}
    if budgets:
        doc.update({"budget_bits": list(budgets)})
    if budgets or args.gptq:
        doc.update({"calib_io": calib_io, "calib_split": args.calib_split, "calib_max_samples": args.calib_max_samples})
    if args.gptq:
        doc.update({"gptq_damp": args.gptq_damp})
    if transpose:
        doc.update({"transpose": True})
    (out_dir / "layer_output_error.json").write_text(json.dumps(doc, indent=2))
    print(f"\nwrote {out_dir / 'layer_output_error.csv'} and {out_dir / 'layer_output_error.json'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
