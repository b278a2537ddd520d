#!/usr/bin/env python3
"""Generate tests/golden/f17_fp4_proxy.npz + golden_meta_f17.json by IMPORTING the reference's mxfp4 / nvfp4 proxies
(quantization_formats.py:171-183,257-278, one Python call per element) — the pattern of make_golden_transpose.py.

Run in the build container only:  python tests/golden/make_golden_fp4_proxy.py
The reference never travels; only the arrays written here are committed.  `x` holds about 200 k float32 inputs chosen where the
proxies have edges (see inputs()); `mxfp4` / `nvfp4` hold the reference's y bits (uint32).  Two recipe tensors of tests/inputs.py
(bf16-valued and float32) are stored as recipes with the reference's pcc / mae / atol per format (pcc64 / mae64 / atol32, as in
golden_meta_r2.json).
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

REF = "/root/reference"
sys.dont_write_bytecode = True
_spec = importlib.util.spec_from_file_location("ref_quantization_formats", f"{REF}/quantization_formats.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

sys.path.insert(1, str(Path(__file__).resolve().parents[2]))
from tests.inputs import gen  # noqa: E402

OUT = Path(__file__).resolve().parent
FORMATS = ["mxfp4", "nvfp4"]
RECIPES = [("normal_bf16", 1717, (96, 160)), ("heavy_f32", 1718, (64, 136))]
MIDPOINTS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])


def _bits(u) -> np.ndarray:
    return np.asarray(u, dtype=np.int64).astype(np.uint32).view(np.float32)


def _around(centres: np.ndarray, n: int) -> np.ndarray:
    """The float32 values within n ulps of every finite positive centre (stepping through the bit patterns)."""
    with np.errstate(over="ignore"):
        c = np.asarray(centres, dtype=np.float32)
    c = c[np.isfinite(c) & (c > 0)].view(np.uint32).astype(np.int64)
    u = (c[:, None] + np.arange(-n, n + 1)[None, :]).ravel()
    return _bits(u[(u >= 0) & (u < 0x7F800000)])


def inputs() -> np.ndarray:
    binades = np.arange(0, 255, dtype=np.int64) << 23
    m = np.concatenate([np.arange(64), np.arange((1 << 23) - 64, 1 << 23)])
    edges = _bits((binades[:, None] | m[None, :]).ravel())                      # first / last 64 mantissas of every binade
    s_edges = _bits((binades[:, None] | np.concatenate([np.arange(24), np.arange((1 << 23) - 48, 1 << 23)])[None, :]).ravel())
    with np.errstate(over="ignore"):
        a6 = (s_edges.astype(np.float64) * 6.0).astype(np.float32)
    a_of_s = _around(a6, 2)    # a whose s = a / 6 sits at a binade edge of s
    sq_mx = _bits([(c + 127) << 23 if c >= -126 else 1 << (c + 149) for c in range(-149, 127)])
    sq_nv = np.unique(ref.quantize_fp8_e4m3(np.concatenate([_bits(np.arange(0x3A000000, 0x43800000, 1 << 19)), [240.0]]).astype(np.float32)))
    sq_nv = sq_nv[sq_nv > 0]
    mids = _around(np.concatenate([(MIDPOINTS[:, None] * sq.astype(np.float64)[None, :]).ravel() for sq in (sq_mx, sq_nv)]), 48)
    rng = np.random.default_rng(17)
    nv_sub = (rng.uniform(6 * 2.0 ** -11, 6 * 2.0 ** -5, 6000)).astype(np.float32)   # nvfp4's subnormal scales (s < 2^-6) and the edge
    nv_top = np.concatenate([_around(np.float32([6 * 248.0, 6 * 256.0, 6 * 240.0, 1535.99988, 1535.99976]), 96),
                             rng.uniform(1400.0, 1600.0, 4000).astype(np.float32)])   # s in [240, 256]
    top = _bits(rng.integers(0x7E800000, 0x7F800000, 2000))                       # the top binades
    special = np.float32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1e-40, 2.0 ** -126, 3.4028235e38, 6 * 2.0 ** -10])
    normal = (rng.standard_normal(4000) * 0.02).astype(np.float32)
    mags = np.unique(np.concatenate([edges, a_of_s, mids, nv_sub, nv_top, top, np.abs(normal)]).view(np.uint32)).view(np.float32)
    signs = np.where(rng.random(mags.size) < 0.5, np.float32(-1.0), np.float32(1.0))
    return np.concatenate([special, mags * signs, normal]).astype(np.float32)


def pearson64(a: np.ndarray, b: np.ndarray) -> float:
    """Two-pass float64 Pearson (make_golden.py)."""
    a = a.astype(np.float64).ravel()
    b = b.astype(np.float64).ravel()
    am, bm = a - a.mean(), b - b.mean()
    den = float(np.sqrt(np.dot(am, am) * np.dot(bm, bm)))
    return 1.0 if den == 0.0 and np.max(np.abs(a - b)) == 0 else (float(np.dot(am, bm)) / den if den else 0.0)


def main() -> None:
    x = inputs()
    f17 = {"x": x.view(np.uint32)}
    with np.errstate(all="ignore"):
        for fmt in FORMATS:
            f17[fmt] = np.ascontiguousarray(ref.quantize_weight_values(x, fmt), dtype=np.float32).view(np.uint32)
    np.savez_compressed(OUT / "f17_fp4_proxy.npz", **f17)
    meta = {"inputs": int(x.size), "formats": FORMATS, "recipes": []}
    for kind, seed, shape in RECIPES:
        t = gen(kind, seed, shape)
        entry = {"kind": kind, "seed": seed, "shape": list(shape), "x_sha256": hashlib.sha256(t.tobytes()).hexdigest(), "formats": {}}
        for fmt in FORMATS:
            with np.errstate(all="ignore"):
                y = np.ascontiguousarray(ref.quantize_weight_values(t, fmt), dtype=np.float32)
            diff = np.abs(t - y)
            entry["formats"][fmt] = {"y_sha256": hashlib.sha256(y.tobytes()).hexdigest(), "pcc64": pearson64(t, y),
                                     "mae64": float(np.mean(diff.astype(np.float64))), "atol32": float(np.max(diff))}
        meta["recipes"].append(entry)
    (OUT / "golden_meta_f17.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(f"f17: {x.size} inputs x {len(FORMATS)} formats; recipes {RECIPES}")


if __name__ == "__main__":
    main()
