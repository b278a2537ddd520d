"""Host (`--backend emulation`) mirror of the reference's quantization_formats.py: bf16 RNE round-trip,
TTNN-style BFP{8,4,2} with one shared exponent per 16 contiguous last-axis elements, fp0, and the
scalar mxfp4 / nvfp4 proxies.  Reference: quantization_formats.py:8,10-26,29-45,71-81,84-164,167-278.

This module is plain NumPy and runs without a GPU.  The `hip` backend does NOT route through it:
it calls libmtq_hip.so (see compression_algorithms/quantizer.py).
"""
from __future__ import annotations

import numpy as np

# The mixed-tile formats and fp0, in the order of their row format codes 0..4 (and of include/mtq.h's MTQ_FMT_*): the formats of
# the layer-output error (output_error.py), which has no proxy rows.
BASE_FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
# Scalar proxies of MXFP4 / NVFP4 (reference :174-183,257-278): elementwise, quantize-only, row format codes 5 and 6.
PROXY_FORMATS = ["mxfp4", "nvfp4"]
ROW_FORMATS = BASE_FORMATS + PROXY_FORMATS   # row format code = index
SUPPORTED_FORMATS = ["mxfp4", "nvfp4", "bf16", "bfp8", "bfp4", "bfp2", "fp0"]   # reference :8, the order of the default list
_MANT_BITS = {"bfp8": 7, "bfp4": 3, "bfp2": 1}


def fp32_to_bf16_round_to_nearest_even(x: np.ndarray) -> np.ndarray:
    """reference :29-35 — RNE on the raw word, uint32 wrap, no NaN special case."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_fp32(bf16: np.ndarray) -> np.ndarray:
    """reference :38-41."""
    return (np.asarray(bf16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def quantize_dequantize_bf16(x: np.ndarray) -> np.ndarray:
    return bf16_to_fp32(fp32_to_bf16_round_to_nearest_even(x))


def quantize_dequantize_bfp_ttnn(x: np.ndarray, mant_bits: int) -> np.ndarray:
    """reference :84-164.  Groups = 16 contiguous last-axis elements aligned from index 0; a partial
    last group is completed with +0.0 (the 32x32 tile of the reference only adds zero padding)."""
    x = np.asarray(x, dtype=np.float32)
    if x.size == 0:
        return x.astype(np.float32)
    shape = x.shape
    rows = x.reshape(1, -1) if x.ndim <= 1 else x.reshape(-1, shape[-1])
    n, w = rows.shape
    wp = -(-w // 16) * 16
    u = np.zeros((n, wp), dtype=np.uint32)
    u[:, :w] = rows.view(np.uint32)
    g = u.reshape(n, wp // 16, 16)
    m = mant_bits
    exp = (g >> np.uint32(23)) & np.uint32(0xFF)
    shared = exp.max(axis=-1, keepdims=True)                      # :118-119
    d = shared - exp                                               # :126
    man = (g & np.uint32(0x7FFFFF)) | np.uint32(1 << 23)           # :121,125
    man = np.where(d > 31, np.uint32(0), man >> np.minimum(d, np.uint32(31)))  # :127-131
    shift = np.uint32(24 - m)
    rv = man & np.uint32((1 << (24 - m)) - 1)                      # :136
    tie = np.uint32(1 << (23 - m))
    man = man >> shift                                             # :137
    up = (rv > tie) | ((rv == tie) & ((man & np.uint32(1)) == 1))  # :138-139
    man = np.minimum(man + up.astype(np.uint32), np.uint32((1 << m) - 1))  # :140-141 saturate
    man = np.where(exp == 0, np.uint32(0), man)                    # :145
    sign = np.where(man == 0, np.uint32(0), g >> np.uint32(31))    # :143
    msb = np.zeros_like(man)
    for b in range(m):                                             # decode table :71-81 as msb search
        msb = np.where(((man >> np.uint32(b)) & np.uint32(1)) == 1, np.uint32(b), msb)
    sc = np.uint32(m - 1) - msb
    ms = (man << (sc + np.uint32(1))) & np.uint32((1 << m) - 1)
    exp_out = shared - sc                                          # :154 (uint32 wrap kept)
    bits = (sign << np.uint32(31)) | (exp_out << np.uint32(23)) | (ms << np.uint32(23 - m))  # :158
    bits = np.where(man == 0, np.uint32(0), bits).astype(np.uint32)
    return bits.reshape(n, wp)[:, :w].copy().view(np.float32).reshape(shape)


def quantize_fp0(x: np.ndarray) -> np.ndarray:
    return np.zeros_like(np.asarray(x, dtype=np.float32), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# mxfp4 / nvfp4 proxies.  y = sign(x) · g(|x|), g(a) = the reference's 32- / 16-element block of identical values a, scaled, quantised
# to e2m1 and back.  The scale's exponent comes from NumPy's float32 log2 (:218, :253), which is correctly rounded: it returns an
# integer for the first few mantissas above a power of two and the last few below one, so floor / ceil of it differ from the exponent
# bits there.  _log2_floor_ceil reproduces that from the bits alone (csrc/mtq_fp4_proxy.hip uses the same rule).
# ---------------------------------------------------------------------------------------------------------------------------------
_FP4_LEVELS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)   # reference :10
# floor(2^j · ln 2) for j = -2..7 (index j + 2): the number of mantissa steps (of 2^-23 relative) next to an integer power of two whose
# log2 lies within half a float32 ulp of that integer
_LOG2_EDGE = np.array([0, 0, 0, 1, 2, 5, 11, 22, 44, 88], dtype=np.int64)
_CHUNK = 1 << 20


def _ulp_log(k: np.ndarray, below: np.ndarray) -> np.ndarray:
    """floor(log2 |k|), minus 1 where the float32 spacing next to |k| on the side the log2 approaches from is the finer one (|k| a power
    of two approached from below).  k != 0."""
    ak = np.abs(k)
    e = np.floor(np.log2(np.maximum(ak, 1))).astype(np.int64)   # exact for these small integers
    return e - (below & ((ak & (ak - 1)) == 0)).astype(np.int64)


def _log2_floor_ceil(s: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(floor, ceil) of np.log2(s) in float32 for finite float32 s > 0, from the bits: s = 2^k · (1 + mn · 2^-23) (subnormals
    normalised).  log2 rounds to k when 1 <= mn <= _LOG2_EDGE[j_lo + 1], to k + 1 when 2^23 - mn <= _LOG2_EDGE[j_hi + 2]."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    eb, man = u >> 23, u & 0x7FFFFF
    sub = eb == 0
    p = np.where(sub, np.floor(np.log2(np.maximum(man, 1))).astype(np.int64), 23)   # subnormal: bit length of the mantissa - 1
    k = np.where(sub, p - 149, eb - 127)
    mn = np.where(sub, (man - (np.int64(1) << p)) << (23 - p), man)
    kk = np.where(k == 0, 1, k)
    jlo = _ulp_log(kk, kk < 0)                 # log2 = k + t moves away from k: up for k > 0, down in magnitude for k < 0
    low = (k != 0) & (mn >= 1) & (mn <= _LOG2_EDGE[np.clip(jlo + 1, 0, 9)])
    K = k + 1
    KK = np.where(K == 0, 1, K)
    jhi = _ulp_log(KK, KK > 0)                 # log2 = K - t' approaches K from below
    high = (K != 0) & ((1 << 23) - mn <= _LOG2_EDGE[np.clip(jhi + 2, 0, 9)])
    floor = np.where(high, K, k)
    ceil = np.where((mn == 0) | low, k, K)
    return floor, ceil


def _pow2_f32(c: np.ndarray) -> np.ndarray:
    """2^c as float32 for -149 <= c <= 127."""
    c = np.asarray(c, dtype=np.int64)
    bits = np.where(c >= -126, (c + 127) << 23, np.int64(1) << np.clip(c + 149, 0, 22))
    return bits.astype(np.uint32).view(np.float32)


def _fp4_nearest(v: np.ndarray) -> np.ndarray:
    """reference :21-26,197-202 — sign(v) · the level of least float32 |v − level|, the first on a tie; chunked."""
    v = np.asarray(v, dtype=np.float32)
    out = np.empty_like(v)
    fv, fo = v.reshape(-1), out.reshape(-1)
    for i in range(0, fv.size, _CHUNK):
        c = fv[i:i + _CHUNK]
        fo[i:i + _CHUNK] = np.sign(c) * _FP4_LEVELS[np.argmin(np.abs(c[:, None] - _FP4_LEVELS[None, :]), axis=-1)]
    return out


def quantize_mxfp4_proxy(x: np.ndarray) -> np.ndarray:
    """reference :174-178 with simulate_mxfp4_amax (:257-266) vectorised: s = float32(a / 6.0 in double), s_q = 2^ceil(log2 s)
    (:249-254; 0 when s = 0), g = fp4(a / s_q) · s_q in float32."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x)
    with np.errstate(all="ignore"):
        s = (a.astype(np.float64) / 6.0).astype(np.float32)
        ok = np.isfinite(s) & (s > 0)
        sq = np.where(np.isinf(s), np.float32(np.inf), np.float32(0.0)).astype(np.float32)
        if np.any(ok):
            sq[ok] = _pow2_f32(_log2_floor_ceil(s[ok])[1])
        g = _fp4_nearest(a / sq) * sq
        g = np.where(a == 0, np.float32(0.0), g)   # :260-261
        return (np.sign(x) * g).astype(np.float32)


def _e4m3_reference(s: np.ndarray) -> np.ndarray:
    """reference :205-246 (e_max = 7, largest value 240) for float32 s >= 0, with floor(log2 s) from _log2_floor_ceil."""
    out = np.zeros_like(s, dtype=np.float32)
    out[np.isinf(s)] = np.inf   # floor(log2 inf) cast to int32 lands in the subnormal branch: round(inf / step) · step
    ok = np.isfinite(s) & (s > 0)
    if not np.any(ok):
        return out
    sv = s[ok]
    e = _log2_floor_ceil(sv)[0]
    r = np.zeros_like(sv)
    big, sub = e > 7, e < -6
    normal = ~big & ~sub
    r[big] = np.float32(240.0)
    step = np.float32(2.0 ** -9)
    r[sub] = np.round(sv[sub] / step) * step
    en = e[normal]
    m = sv[normal].astype(np.float64) / np.exp2(en.astype(np.float64))
    fq = np.round((m - 1.0) * 8.0) / 8.0
    bumped = fq >= 1.0
    fq = np.where(bumped, 0.0, fq)
    en = np.where(bumped, np.minimum(en + 1, 7), en)
    r[normal] = ((1.0 + fq) * np.exp2(en.astype(np.float64))).astype(np.float32)
    out[ok] = r
    return out


def quantize_nvfp4_proxy(x: np.ndarray) -> np.ndarray:
    """reference :179-183 with simulate_nvfp4_amax (:269-278) vectorised: s = float32(a) / 6.0 in float32 (0 unless a > 0),
    s_q = the reference's e4m3 of s, g = fp4(a / s_q) · s_q in float32 (0 when s_q = 0)."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x)
    with np.errstate(all="ignore"):
        s = np.where(a > 0, a / np.float32(6.0), np.float32(0.0)).astype(np.float32)
        sq = _e4m3_reference(s)
        g = _fp4_nearest(a / sq) * sq
        g = np.where(sq == 0, np.float32(0.0), g)   # :274-275
        return (np.sign(x) * g).astype(np.float32)


def quantize_weight_values(x: np.ndarray, fmt: str) -> np.ndarray:
    """reference :171-194."""
    fmt = fmt.lower()
    x = np.asarray(x, dtype=np.float32)
    if fmt == "mxfp4":
        return quantize_mxfp4_proxy(x)
    if fmt == "nvfp4":
        return quantize_nvfp4_proxy(x)
    if fmt == "bf16":
        return quantize_dequantize_bf16(x)
    if fmt in _MANT_BITS:
        return quantize_dequantize_bfp_ttnn(x, mant_bits=_MANT_BITS[fmt])
    if fmt == "fp0":
        return quantize_fp0(x)
    raise ValueError(f"Unsupported weight format: {fmt}")
