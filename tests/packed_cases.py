"""Inputs shared by the packed test modules: the specials tensor, seeded maps, the expected reconstruction from the oracle, and the
integer-grid case of the linear tests with its preconditions."""
from __future__ import annotations

import numpy as np

from oracle import mtq_oracle as orc

FORMATS = ["bf16", "bfp8", "bfp4", "bfp2"]
TILE_BYTES = (2048, 1088, 576, 320)
GRID = 2.0 ** -8


def specials(shape, seed: int = 11) -> np.ndarray:
    """float32 words with every exponent field 1..254 present, groups whose exponents spread over the whole range (the d > 31 wrap of
    the alignment shift), groups at the two ends of the range, and zeros, -0, ±Inf, NaNs of both signs and denormals sprinkled in."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    exp = rng.integers(1, 255, size=n).astype(np.uint32)
    exp[: min(n, 254)] = (np.arange(min(n, 254)) % 254 + 1).astype(np.uint32)        # every field at least once
    third = n // 3
    exp[third: third + third // 2] = rng.integers(1, 9, size=third // 2).astype(np.uint32)           # the bottom of the range
    exp[third + third // 2: 2 * third] = rng.integers(247, 255, size=2 * third - third - third // 2).astype(np.uint32)
    u = (rng.integers(0, 2, size=n).astype(np.uint32) << np.uint32(31)) | (exp << np.uint32(23)) | rng.integers(0, 1 << 23, size=n).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF,
                        0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x3F808000, 0x3F818000, 0x7F7F8000], dtype=np.uint32)
    where = rng.choice(n, size=min(n, max(16, n // 7)), replace=False)
    u[where] = special[np.arange(where.size) % special.size]
    return u.view(np.float32).reshape(shape)


def random_map(shape2d, seed: int) -> np.ndarray:
    th, tw = orc.tiles_hw(*shape2d)
    return np.random.default_rng(seed).integers(0, 4, size=(th, tw)).astype(np.int8)


def uniform_map(shape2d, code: int) -> np.ndarray:
    th, tw = orc.tiles_hw(*shape2d)
    return np.full((th, tw), code, dtype=np.int8)


def expected_bits(x: np.ndarray, amap: np.ndarray) -> np.ndarray:
    """uint32 words of the reconstruction, in x's shape: per tile, the oracle's quantize_weight_values of the tile's format over the
    2-D flatten (groups never cross a tile: whole-tensor quantisation is tile-wise quantisation)."""
    x2d, info = orc.flatten_2d(np.asarray(x, dtype=np.float32))
    h, w = x2d.shape
    sel = np.repeat(np.repeat(amap, 32, axis=0), 32, axis=1)[:h, :w]
    y = np.zeros((h, w), dtype=np.uint32)
    for code in np.unique(amap):
        q = orc.quantize_weight_values(x2d, FORMATS[int(code)]).view(np.uint32)
        y = np.where(sel == code, q, y)
    if info[0] == "scalar":
        return y.reshape(())
    if info[0] == "vector":
        return y.reshape(-1)[: info[1]]
    return y.reshape(info[1])


def stream_bytes(amap: np.ndarray) -> int:
    return int(sum(int((amap == c).sum()) * TILE_BYTES[c] for c in range(4)))


def _grid_case(m, n, k, seed):
    """The integer grid: X integers |x| <= 4, W and the bias on the 2^-8 grid with |w| < 1."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(m, k)).astype(np.float32)
    w = (rng.integers(-255, 256, size=(n, k)) * GRID).astype(np.float32)
    b = (rng.integers(-255, 256, size=(n,)) * GRID).astype(np.float32)
    return x, w, b


def _grid_preconditions(x, what, b):
    assert np.all(np.abs(x) <= 4) and np.array_equal(x, np.round(x))
    assert np.array_equal(what / GRID, np.round(what / GRID)) and np.array_equal(b / GRID, np.round(b / GRID))
    worst = (np.abs(x).astype(np.float64) @ np.abs(what).T + np.abs(b)[None, :]) / GRID
    assert worst.max() < 2.0 ** 24
