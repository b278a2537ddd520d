#!/usr/bin/env python3
"""Generate tests/golden/f15_transpose.npz + golden_meta_f15.json by IMPORTING the reference's `transpose` algorithm
(compression_algorithms/transpose.py) with its emulation Quantizer — the pattern of make_golden.py.

Run in the build container only:  python tests/golden/make_golden_transpose.py
The reference never travels; only the arrays written here are committed.  Small inputs are stored with the reference's y bits
(uint32) per format; the 1024x4096 bf16-valued tensor is stored as a recipe (tests/inputs.py::gen) with the SHA-256 of every
format's y and the reference's float32 pcc / mae / atol (metrics.py).
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

sys.path.insert(1, str(Path(__file__).resolve().parents[2]))
from tests.inputs import gen, to_bf16_valued  # noqa: E402

OUT = Path(__file__).resolve().parent
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
BIG = ("normal_bf16", 1515, (1024, 4096))


def specials() -> np.ndarray:
    """(40, 24) float32: ±Inf, NaN, ±0, denormals, 2^127-scale values, and column groups (16 rows of one column) whose exponent
    spread exceeds 31, among ordinary values."""
    rng = np.random.default_rng(15)
    x = (rng.standard_normal((40, 24)) * 0.02).astype(np.float32)
    x[3, 0], x[20, 0] = np.inf, -np.inf
    x[5, 1] = np.nan
    x[0:16, 2] = 0.0
    x[7, 2] = -0.0
    x[0:16, 3] = np.float32(1e-40) * np.arange(1, 17, dtype=np.float32)          # denormal-only group
    x[16:32, 3] = np.float32(1e-39)
    x[17, 3] = 0.5                                                             # denormals under a normal maximum
    x[0:16, 4] = np.float32(2.0 ** 127) * np.linspace(1, 1.9, 16, dtype=np.float32)
    x[16:32, 4] = -np.float32(1.5 * 2.0 ** 127)
    x[0, 5], x[1:16, 5] = 1.0, np.float32(2.0 ** -40)                          # spread 40 > 31
    x[16, 6], x[17:32, 6] = -3.0e20, np.float32(7.0e-20)                       # spread > 31, negative maximum
    x[32:40, 7] = np.float32(2.0 ** -126)                                      # smallest normal, short last group
    x[9, 8] = np.float32(3.4028235e38)                                         # float32 max: saturating round-up
    return x


def reference_run(x: np.ndarray) -> list:
    with tempfile.TemporaryDirectory() as tmp:
        cache = CacheContext(root=Path(tmp), tensor_name="t", backend="emulation", recompute=True, run_tag="golden")
        res = create_algorithm("transpose", {}).run(x, FORMATS, Quantizer("emulation"), cache)
    assert [r.fmt for r in res] == [f.upper() for f in FORMATS] and all(r.compression == "transpose" for r in res)
    return res


def main() -> None:
    rng = np.random.default_rng(2015)
    cases = {
        "s96x80": (rng.standard_normal((96, 80)) * 0.02).astype(np.float32),
        "s33x47": (rng.standard_normal((33, 47)) * 0.05).astype(np.float32),
        "v37": (rng.standard_normal(37) * 0.1).astype(np.float32),
        "scalar": np.asarray(np.float32(0.3125)),
        "s3x20x35": (rng.standard_normal((3, 20, 35)) * 0.02).astype(np.float32),
        "s1000x3": (rng.standard_normal((1000, 3)) * np.exp(rng.standard_normal((1000, 3)))).astype(np.float32),
        "specials": specials(),
        "bf16_256x192": to_bf16_valued((rng.standard_normal((256, 192)) * 0.02).astype(np.float32)),
    }
    f15 = {}
    for name, x in cases.items():
        f15[f"{name}__x"] = x
        with np.errstate(all="ignore"):
            res = reference_run(x)
        for fmt, r in zip(FORMATS, res):
            y = np.asarray(r.y, dtype=np.float32)
            assert y.shape == x.shape
            f15[f"{name}__{fmt}"] = np.ascontiguousarray(y).view(np.uint32)
    np.savez_compressed(OUT / "f15_transpose.npz", **f15)

    big = gen(*BIG)
    res = reference_run(big)
    meta = {"cases": list(cases), "formats": FORMATS, "big": {"kind": BIG[0], "seed": BIG[1], "shape": list(BIG[2]),
                                                               "x_sha256": hashlib.sha256(big.tobytes()).hexdigest(), "formats": {}}}
    for fmt, r in zip(FORMATS, res):
        y = np.ascontiguousarray(np.asarray(r.y, dtype=np.float32))
        diff = np.abs(big - y)
        meta["big"]["formats"][fmt] = {"y_sha256": hashlib.sha256(y.tobytes()).hexdigest(), "pcc": float(pearson_corr(big, y)),
                                       "mae": float(np.mean(diff)), "atol": float(np.max(diff))}
    (OUT / "golden_meta_f15.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(f"f15: {len(cases)} cases x {len(FORMATS)} formats; big {BIG}")


if __name__ == "__main__":
    main()
