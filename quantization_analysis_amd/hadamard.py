"""Block Hadamard rotation along the reduction axis.

For a layer y = x·Wᵀ and the orthonormal block-diagonal H (one Sylvester–Hadamard block H_B · 2^(−p/2) per B = 2^p consecutive k),
y = (x·H)·(W·H)ᵀ: rotating W offline and x online leaves the layer unchanged in exact arithmetic and spreads an outlier channel over
the B channels of its block, out of the 16-value shared-exponent groups whose error one outlier decides.

Contract (both backends): every aligned block of B consecutive elements along the last axis becomes fl32(S · c_p), S = block · H_B with
H_B in natural (Sylvester) order and c_p = float32(2^(−p/2)); the result is float32, or bf16 by round-to-nearest-even of that float32.
32 <= B <= 4096, B a power of two dividing k.
  * emulation — S by float64 butterflies on the host, one rounding of S · float64(c_p) to float32: the oracle;
  * hip       — csrc/mtq_hadamard.hip (mtq_hadamard_rows): p stages of float32 butterflies, stride 1 first, then the one multiply.  Where
                every partial sum is exact in float32 (small-integer inputs) the two agree bit for bit; otherwise each output is within
                (p + 2) · 2⁻²⁴ · c_p · Σ|x_i| of the oracle.  With q_fmt the same launch also writes the BFP image of its bf16 output.
"""
from __future__ import annotations

import math

import numpy as np

MIN_BLOCK, MAX_BLOCK = 32, 4096
BACKENDS = ("emulation", "hip")


def check_block(k: int, block: int) -> int:
    """block as an int, or ValueError: a power of two in [32, 4096] that divides k."""
    block, k = int(block), int(k)
    if block < MIN_BLOCK or block > MAX_BLOCK or block & (block - 1):
        raise ValueError(f"rotation block must be a power of two in [{MIN_BLOCK}, {MAX_BLOCK}], got {block}")
    if k <= 0 or k % block:
        raise ValueError(f"rotation block {block} does not divide k = {k}")
    return block


def auto_block(k: int) -> int:
    """The largest power of two dividing k, capped at 4096 (7168 → 1024, 14336 → 2048); ValueError when that is below 32."""
    k = int(k)
    b = min(k & -k, MAX_BLOCK) if k > 0 else 0
    if b < MIN_BLOCK:
        raise ValueError(f"k = {k} has no power-of-two factor of at least {MIN_BLOCK} to rotate by")
    return b


def scale(block: int) -> np.float32:
    """c_p = float32(2^(−p/2)) for block = 2^p."""
    p = int(block).bit_length() - 1
    return np.float32(math.ldexp(math.sqrt(0.5) if p & 1 else 1.0, -(p // 2)))


def _round_bf16(y32: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(y32, dtype=np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)).view(np.float32)


def hadamard_emulation(x, block: int, out_dtype=None):
    """The oracle: x (ndarray or tensor, any leading axes) → a torch tensor of x's shape in out_dtype (torch.float32 when None, or
    torch.bfloat16), on the host."""
    import torch

    a = np.asarray(x.detach().float().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
    block = check_block(a.shape[-1], block)
    s = a.reshape(-1, block).copy()
    h = 1
    while h < block:
        v = s.reshape(-1, block // (2 * h), 2, h)
        lo, hi = v[:, :, 0, :] + v[:, :, 1, :], v[:, :, 0, :] - v[:, :, 1, :]
        v[:, :, 0, :], v[:, :, 1, :] = lo, hi
        h *= 2
    y = (s * np.float64(scale(block))).astype(np.float32).reshape(a.shape)
    out_dtype = out_dtype or torch.float32
    if out_dtype == torch.bfloat16:
        return torch.from_numpy(_round_bf16(y)).to(torch.bfloat16)
    if out_dtype != torch.float32:
        raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    return torch.from_numpy(y)


def hadamard(x, block: int, out_dtype=None, backend: str = "emulation", q_fmt=None):
    """x rotated along its last axis → a tensor of x's shape in out_dtype (x's dtype when None; float32 for other inputs).  hip: x is
    moved to the current device and the result stays there; q_fmt (bfp8 / bfp4 / bfp2, hip only) returns (y, Q(y)) from one launch."""
    import torch

    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {', '.join(BACKENDS)}")
    block = check_block(x.shape[-1], block)
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float32) else torch.float32
    if backend == "emulation":
        if q_fmt is not None:
            raise ValueError("q_fmt is the hip kernel's second output")
        return hadamard_emulation(x, block, out_dtype)
    from . import hip_backend as hb

    xd = x.to(torch.device("cuda", torch.cuda.current_device()))
    xd = xd if xd.dtype in (torch.bfloat16, torch.float32) else xd.float()
    x2 = xd.reshape(-1, xd.shape[-1])
    x2 = x2 if x2.stride(-1) == 1 else x2.contiguous()
    got = hb.hadamard_rows(x2, block, out_dtype=out_dtype, q_fmt=q_fmt)
    if q_fmt is None:
        return got.view(xd.shape)
    return got[0].view(xd.shape), got[1].view(xd.shape)


def rotate_weight(w, block: int, axis: int = -1, backend: str = "emulation"):
    """W′ = W·H as float32, rotated along `axis` of a 2-D weight: the last axis for an (n, k) weight, axis 0 for a (k, n) one (through a
    transposed copy: this runs offline)."""
    if w.dim() != 2 or axis not in (-1, 0, 1):
        raise ValueError("rotate_weight takes a 2-D weight and axis -1, 0 or 1")
    import torch

    if axis == 0:
        return rotate_weight(w.T.contiguous(), block, -1, backend).T.contiguous()
    return hadamard(w if w.dtype in (torch.bfloat16, torch.float32) else w.float(), block, torch.float32, backend)
