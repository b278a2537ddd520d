#!/usr/bin/env python3
"""Pack a tensor under a mixed-tile assignment map into the packed format of include/mtq.h, and unpack it again.

  pack   MODEL TENSOR ASSIGNMENT --out file.npz [--backend hip|emulation] [--verify] [--layout transpose --store-transposed]
         prints the packed bytes, the size model's bytes (tile_utils.mixed_tile_total_bytes) and both ratios to bf16; --verify
         unpacks the stream and compares it bit for bit with the reconstruction of reconstruct_mixed_tile_assignment.py (a mismatch
         exits non-zero).
  unpack file.npz --out y.npy [--backend hip|emulation] [--transposed]
         writes the float32 tensor the stream holds; --transposed writes its transpose, the orientation of the weight that was packed
         with --store-transposed.

The packed format is the row layout; a map written for --layout transpose is refused on its own.  With --store-transposed the 2-D
tensor's TRANSPOSE is packed under that map (packed.pack_transposed: a transposed-layout map of W is a row-layout map of Wᵀ), the file
holds an ordinary row-layout tensor of shape (k, n) for packed.matmul, and --verify compares packed.unpack_transposed with what
reconstruct_mixed_tile_assignment.py --layout transpose gives."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np

from quantization_analysis_amd import packed
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import TileStats, reconstruct
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS, flatten_2d, mixed_tile_total_bytes
from quantization_analysis_amd.hip_backend import MtqError
from quantization_analysis_amd.model_source import build_model_index


def _reconstruction(x, a: np.ndarray, backend: str, transposed: bool = False) -> np.ndarray:
    """What scripts/reconstruct_mixed_tile_assignment.py writes for the row layout, or (transposed, a 2-D x) for --layout transpose."""
    quantizer = Quantizer(backend)
    if backend == "hip":
        from quantization_analysis_amd import hip_backend as hb

        x2d, info = hb.to_device_2d(x)
        if transposed:   # X read in place, records and map over Xᵀ's grid (K3T)
            th, tw = hb.tiles_hw(x2d.shape[1], x2d.shape[0])
            ts = TileStats(0, th, tw, int(x.numel()), ("nd", tuple(x2d.shape[::-1])), x2d, "hip", True, transposed=True)
        else:
            th, tw = hb.tiles_hw(*x2d.shape)
            ts = TileStats(0, th, tw, int(x.numel()), info, x2d, "hip", True)
    else:
        xf = x.float().numpy()
        x2d, info = flatten_2d(np.transpose(xf) if transposed else xf)
        th, tw = -(-x2d.shape[0] // 32), -(-x2d.shape[1] // 32)
        ts = TileStats(0, th, tw, int(xf.size), info, x2d, backend, True)
    y = np.asarray(reconstruct(ts, a.astype(np.int8), quantizer), dtype=np.float32)
    return np.ascontiguousarray(y.T) if transposed else y


def _pack(args) -> int:
    index = build_model_index(args.repo_or_url, revision=args.revision)
    a = np.load(args.assignment)
    if args.assignment_mapping:
        names = json.loads(Path(args.assignment_mapping).read_text()).get("int_to_format", MIXED_TILE_FORMATS)
        a = np.vectorize(lambda v: MIXED_TILE_FORMATS.index(names[int(v)]))(a)
    x = index.load(args.tensor_name)
    transposed = bool(args.store_transposed)
    if transposed and args.layout != "transpose":
        print("error: --store-transposed packs the tensor's transpose under a map written for --layout transpose; pass both")
        return 1
    try:
        if transposed:
            pt = packed.pack_transposed(x, a, backend=args.backend)
        else:
            pt = packed.pack(x, a, backend=args.backend, layout=args.layout)
    except MtqError as exc:
        print(f"error: {exc}" + (" (--store-transposed packs the transpose of a 2-D tensor under such a map)" if args.layout == "transpose" and not transposed else ""))
        return 1
    packed.save(args.out, pt)
    counts = pt.counts()
    model = mixed_tile_total_bytes(counts)
    bf16 = 2.0 * 1024 * pt.map.size
    print(f"wrote {args.out} {pt.shape} tiles {pt.map.shape[0]}x{pt.map.shape[1]} counts {counts}")
    print(f"packed bytes {pt.nbytes} (+ {pt.total_bytes - pt.nbytes} of map and offsets) ratio to bf16 {pt.nbytes / bf16:.5f}")
    print(f"size-model bytes {model:.1f} ratio to bf16 {model / bf16:.5f}")
    if args.verify:
        y = (packed.unpack_transposed if transposed else packed.unpack)(pt, backend=args.backend)
        y = np.asarray(y.cpu().numpy() if args.backend == "hip" else y)
        want = _reconstruction(x, a, args.backend, transposed)
        same = y.shape == want.shape and np.array_equal(np.ascontiguousarray(y).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
        if not same:
            bad = int(np.count_nonzero(np.ascontiguousarray(y).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))) if y.shape == want.shape else -1
            print(f"verify: MISMATCH ({bad} of {want.size} words differ from the reconstruction)")
            return 2
        print(f"verify: ok ({want.size} words equal the reconstruction bit for bit)")
    return 0


def _unpack(args) -> int:
    try:
        pt = packed.load(args.file)
        y = (packed.unpack_transposed if args.transposed else packed.unpack)(pt, backend=args.backend)
    except MtqError as exc:
        print(f"error: {exc}")
        return 1
    y = y.cpu().numpy() if args.backend == "hip" else y
    np.save(args.out, np.asarray(y, dtype=np.float32))
    print(f"wrote {args.out} {np.asarray(y).shape}")
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Pack / unpack a tensor in the packed mixed-tile format.")
    sub = p.add_subparsers(dest="command", required=True)
    pk = sub.add_parser("pack", help="pack a tensor under an assignment map")
    pk.add_argument("repo_or_url")
    pk.add_argument("tensor_name")
    pk.add_argument("assignment", help="Path to assignment .npy file (ints per tile).")
    pk.add_argument("--assignment-mapping", default=None)
    pk.add_argument("--revision", default="main")
    pk.add_argument("--cache-dir", default="data/hf-cache")
    pk.add_argument("--backend", choices=list(packed.BACKENDS), default="emulation")
    pk.add_argument("--layout", choices=["rows", "transpose"], default="rows", help="Tile grid the map was written for; only rows can be packed.")
    pk.add_argument("--store-transposed", action="store_true",
                    help="With --layout transpose: pack the 2-D tensor's transpose under the map (packed.pack_transposed); the file holds a (k, n) row-layout tensor.")
    pk.add_argument("--out", required=True)
    pk.add_argument("--verify", action="store_true")
    pk.set_defaults(fn=_pack)
    up = sub.add_parser("unpack", help="unpack a packed file")
    up.add_argument("file")
    up.add_argument("--backend", choices=list(packed.BACKENDS), default="emulation")
    up.add_argument("--transposed", action="store_true", help="Write the transpose of the stored 2-D tensor (packed.unpack_transposed).")
    up.add_argument("--out", required=True)
    up.set_defaults(fn=_unpack)
    args = p.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    raise SystemExit(main())
