#!/usr/bin/env python3
"""Generate tests/golden/f16_mixed_transpose.npz + golden_meta_f16.json by IMPORTING the reference's mixed-tile searches
(compression_algorithms/mixed_tile_{greedy,threshold,random}.py) with its emulation Quantizer and running them on np.transpose(x) —
the contract of params["layout"] = "transpose" here — in the pattern of make_golden_transpose.py.

Run in the build container only:  python tests/golden/make_golden_mixed_transpose.py
The reference never travels; only the arrays written here are committed.  Per run: the reference's map over the tile grid of
np.transpose(x), tile counts, tile_bytes and y = np.transpose(y_T) — as uint32 bits for small inputs, as a SHA-256 for the 1024x4096
bf16-valued tensor (stored as a tests/inputs.py recipe) — and the float32 pcc / mae / atol wq forms from (x, y).
"""
from __future__ import annotations

import hashlib
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from compression_algorithms import create_algorithm  # noqa: E402  (reference)
from compression_algorithms.cache import CacheContext  # noqa: E402
from compression_algorithms.metrics import pearson_corr  # noqa: E402
from compression_algorithms.quantizer import Quantizer  # noqa: E402
from compression_algorithms.tile_utils import reshape_to_2d_with_padding, tile_metrics  # noqa: E402

sys.path.insert(1, str(Path(__file__).resolve().parents[2]))
from tests.golden.make_golden_transpose import specials  # noqa: E402
from tests.inputs import gen, to_bf16_valued  # noqa: E402

OUT = Path(__file__).resolve().parent
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
MIXED = ["bf16", "bfp8", "bfp4", "bfp2"]
BIG = ("normal_bf16", 1616, (1024, 4096))


def tile_scores_t(x: np.ndarray, fmt: str, metric: str) -> np.ndarray:
    """The reference's float32 per-tile scores of np.transpose(x) in fmt (mixed_tile_threshold.py:97-110)."""
    q = Quantizer("emulation")
    xt = np.transpose(x)
    padded, _, pad = reshape_to_2d_with_padding(xt)
    th, tw = pad[2] // 32, pad[3] // 32
    tr = padded.reshape(th, 32, tw, 32).transpose(0, 2, 1, 3).reshape(-1, 32, 32)
    pq, _, _ = reshape_to_2d_with_padding(q.quantize(xt, fmt))
    tq = pq.reshape(th, 32, tw, 32).transpose(0, 2, 1, 3).reshape(-1, 32, 32)
    return np.asarray(tile_metrics(tr, tq, metric), dtype=np.float32)


def reference_run(x: np.ndarray, alg: str, params: dict):
    with tempfile.TemporaryDirectory() as tmp:
        cache = CacheContext(root=Path(tmp), tensor_name="t", backend="emulation", recompute=True, run_tag="golden")
        with np.errstate(all="ignore"):
            res = create_algorithm(alg, dict(params)).run(np.transpose(x), FORMATS, Quantizer("emulation"), cache)
    assert len(res) == 1 and res[0].fmt == "MIXED"
    r = res[0]
    y = np.ascontiguousarray(np.transpose(np.asarray(r.y, dtype=np.float32)))
    assert y.shape == x.shape
    with np.errstate(all="ignore"):
        diff = np.abs(x - y)
        cols = {"pcc": float(np.float32(pearson_corr(x, y))), "mae": float(np.float32(np.mean(diff))) if diff.size else 0.0,
                "atol": float(np.float32(np.max(diff))) if diff.size else 0.0}
    return y, np.asarray(r.meta["assignment"], dtype=np.int8), [int(r.tile_counts[f]) for f in MIXED], float(r.tile_bytes), cols


def runs_for(name: str, x: np.ndarray) -> list:
    """(run name, algorithm, params) of one input: greedy over seeds and metrics, threshold with knife-edge thresholds, random."""
    out = []
    scale = float(np.nanmax(np.abs(x[np.isfinite(x)]))) if np.isfinite(x).any() else 1.0
    for seed in (1, 7, 123):
        out.append((f"{name}__greedy_pcc_s{seed}", "mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": seed}))
    if name != "specials":   # NaN in x makes the reference's whole-tensor mae / atol NaN: the row-layout search already departs from it there
        out.append((f"{name}__greedy_mae_s5", "mixed-tile-greedy", {"metric": "mae", "threshold": 0.02 * scale, "seed": 5}))
        out.append((f"{name}__greedy_atol_s9", "mixed-tile-greedy", {"metric": "atol", "threshold": 0.06 * scale, "seed": 9}))
    s4 = tile_scores_t(x, "bfp4", "pcc")
    s4 = s4[np.isfinite(s4)]
    if s4.size:
        knife = float(np.sort(s4)[s4.size // 3])
        out.append((f"{name}__thr_pcc_median", "mixed-tile-threshold", {"metric": "pcc", "threshold": round(float(np.median(s4)), 6)}))
        out.append((f"{name}__thr_pcc_knife_eq", "mixed-tile-threshold", {"metric": "pcc", "threshold": knife}))
        out.append((f"{name}__thr_pcc_knife_eps", "mixed-tile-threshold", {"metric": "pcc", "threshold": knife + 1e-9}))
    sm = tile_scores_t(x, "bfp4", "mae")
    sm = sm[np.isfinite(sm)]
    if sm.size:
        out.append((f"{name}__thr_mae_knife_eq", "mixed-tile-threshold", {"metric": "mae", "threshold": float(np.sort(sm)[sm.size // 2])}))
    out.append((f"{name}__random_pcc_s0", "mixed-tile-random", {"metric": "pcc", "threshold": 0.99, "iters": 12, "seed": 0}))
    out.append((f"{name}__random_mae_s5", "mixed-tile-random", {"metric": "mae", "threshold": 0.01 * scale, "iters": 8, "seed": 5}))
    return out


def main() -> None:
    rng = np.random.default_rng(2016)
    cases = {
        "s100x150": (rng.standard_normal((100, 150)) * 0.02).astype(np.float32),
        "s96x160": to_bf16_valued((rng.standard_normal((96, 160)) * np.exp(rng.standard_normal((96, 1)))).astype(np.float32)),
        "v1003": (rng.standard_normal(1003) * 0.1).astype(np.float32),
        "s3x40x72": (rng.standard_normal((3, 40, 72)) * 0.02).astype(np.float32),
        "specials": specials(),
    }
    f16 = {}
    meta = {"cases": list(cases), "formats": FORMATS, "runs": [], "big": None}
    for name, x in cases.items():
        f16[f"{name}__x"] = x
        for run, alg, params in runs_for(name, x):
            y, amap, counts, tile_bytes, cols = reference_run(x, alg, params)
            f16[f"{run}__y"] = y.view(np.uint32)
            f16[f"{run}__map"] = amap
            meta["runs"].append({"run": run, "case": name, "algorithm": alg, "params": params, "counts": counts, "tile_bytes": tile_bytes, **cols})
    np.savez_compressed(OUT / "f16_mixed_transpose.npz", **f16)

    big = gen(*BIG)
    big_runs = [("big__greedy_pcc_s123", "mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": 123})]
    s4 = tile_scores_t(big, "bfp4", "pcc")
    big_runs.append(("big__thr_pcc_knife_eq", "mixed-tile-threshold", {"metric": "pcc", "threshold": float(np.sort(s4)[s4.size // 3])}))
    big_runs.append(("big__random_pcc_s3", "mixed-tile-random", {"metric": "pcc", "threshold": 0.995, "iters": 4, "seed": 3}))
    meta["big"] = {"kind": BIG[0], "seed": BIG[1], "shape": list(BIG[2]), "x_sha256": hashlib.sha256(big.tobytes()).hexdigest(), "runs": []}
    for run, alg, params in big_runs:
        y, amap, counts, tile_bytes, cols = reference_run(big, alg, params)
        meta["big"]["runs"].append({"run": run, "algorithm": alg, "params": params, "counts": counts, "tile_bytes": tile_bytes,
                                    "y_sha256": hashlib.sha256(y.tobytes()).hexdigest(),
                                    "map_sha256": hashlib.sha256(np.ascontiguousarray(amap).tobytes()).hexdigest(),
                                    "map_shape": list(amap.shape), **cols})
    (OUT / "golden_meta_f16.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(f"f16: {len(meta['runs'])} runs over {len(cases)} inputs; big {BIG}: {len(big_runs)} runs")


if __name__ == "__main__":
    main()
