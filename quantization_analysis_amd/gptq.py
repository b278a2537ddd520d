"""GPTQ-style error-compensated BFP weights for the layer-output error (output_error.py, scripts/layer_output_error.py).

Inputs: W is one op's weight, n × k (bf16 or float32, nn.Linear convention); X_cal its calibration activations, m × k bf16 as
layer_io.chunks yields them; `codes` a per-tile code map, int8 [ceil(n/32), ceil(k/32)] over MIXED_TILE_FORMATS (a pure format is the
constant map).  Column j of row r lies in tile (r // 32, j // 32) and in the 16-column group j // 16 of the row layout.

Hessian (host, float64, shared by both backends):
  1. H = X_calᵀX_cal (k × k);
  2. a dead column (H_jj == 0) gets H_jj := 1; W is NOT zeroed there (unlike reference GPTQ): with nothing to compensate, a dead
     column is rounded like RTN;
  3. λ = damp · mean(diag H) (damp finite and > 0, 0.01 by default), H_d = H + λI;
  4. U = the upper Cholesky factor of H_d⁻¹, from torch float64 on the host (CPU LAPACK) for both backends.
  No candidate is made (a reason is returned instead) when the calibration holds no tokens or a Cholesky factorisation fails.

Fixed-exponent element rule q_E(x, f) of a float64 value x:
  * bf16: bf16_round(float32(x));
  * bfp8 / bfp4 / bfp2 (M = 7 / 3 / 1 mantissa bits): the reference's per-element rule (quantization_formats.py) on float32(x) with
    shared exponent E, except that an exponent field above E saturates to ±(2^M − 1)·step with the sign kept (step = 2^(E−126−M)).
  With E = the group's own maximum exponent field, q_E equals quantize_weight_values bit for bit.

Sweep (row-independent, float64): for each row and j = 0 .. k−1 in order:
  1. at the start of a 16-column group, E = the maximum exponent field of float32 of the group's CURRENT values (columns < k only; the
     device pads the last group with zeros instead, whose exponent field 0 never raises a maximum: the same rule);
  2. f = the code of j's tile; q_j = q_E(w_j, f);
  3. e_j = (w_j − q_j) / U_jj;
  4. w_j' −= e_j · U_jj' for every j' > j.
  Ŵ = q (float32: every q lies on its format's grid and bf16(Ŵ) == Ŵ) and loss_r = Σ_j e_rj².  Lazy (blocked) updates change only the
  summation order.  Because Δ = W − Ŵ = E·U, Σ_r δ_r H_d δ_rᵀ = Σ_r loss_r.

Margin (emulation only): per row, over the decisions it makes (each BFP group's E, each element's quantisation level), the least
distance of the float64 value decided to the nearest value that would change that decision, divided by the element's step (its
group's BFP step or its bf16 ulp).  Two routes that agree within a small fraction of a step give the same row where it is clear.

Backends: emulation — NumPy / torch float64 on the host, the oracle of the GPU tests; hip — csrc/mtq_gptq.hip (mtq_gram_full per
chunk, the host factorisation, then mtq_gptq_sweep on the device).
"""
from __future__ import annotations

import math
from typing import Iterable, Union

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS

TILE = 32
GROUP = 16
GPTQ_FORMATS = ("bfp8", "bfp4", "bfp2")
DEFAULT_DAMP = 0.01
_MANT = {1: 7, 2: 3, 3: 1}                     # MIXED_TILE_FORMATS code → mantissa bits


def check_damp(damp) -> float:
    d = float(damp)
    if not (math.isfinite(d) and d > 0.0):
        raise ValueError(f"damp must be finite and > 0, got {damp!r}")
    return d


def constant_codes(n: int, k: int, fmt: str) -> np.ndarray:
    return np.full((-(-n // TILE), -(-k // TILE)), MIXED_TILE_FORMATS.index(fmt), dtype=np.int8)


# ----------------------------------------------------------------------------- element rule

def _exp_field(u: np.ndarray) -> np.ndarray:
    return ((u >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)


def bfp_fixed_bits(u: np.ndarray, shared: np.ndarray, m: int) -> np.ndarray:
    """The reference's BFP element rule on float32 words u with shared exponent `shared` (int, broadcast), M = m, saturating an
    exponent above `shared` to ±(2^m − 1)·step → uint32 words."""
    u = np.asarray(u, dtype=np.uint32)
    e = _exp_field(u)
    E = np.broadcast_to(np.asarray(shared, dtype=np.int64), e.shape)
    d = E - e
    qmax = (1 << m) - 1
    man = ((u & np.uint32(0x7FFFFF)) | np.uint32(1 << 23)).astype(np.int64)
    man = np.where(d > 31, 0, man >> np.clip(d, 0, 31))
    rv = man & ((1 << (24 - m)) - 1)
    tie = 1 << (23 - m)
    man = man >> (24 - m)
    up = (rv > tie) | ((rv == tie) & ((man & 1) == 1))
    man = np.minimum(man + up, qmax)
    man = np.where(e == 0, 0, man)
    man = np.where(d < 0, qmax, man)                              # saturation: exponent field above E
    msb = np.zeros_like(man)
    for b in range(m):
        msb = np.where(((man >> b) & 1) == 1, b, msb)
    sc = (m - 1) - msb
    ms = (man << (sc + 1)) & qmax
    sign = (u >> np.uint32(31)).astype(np.int64)
    bits = ((sign << 31) | ((E - sc) << 23) | (ms << (23 - m))) & 0xFFFFFFFF   # exp_out = E − sc with the reference's uint32 wrap
    return np.where(man == 0, 0, bits).astype(np.uint32)


def _bf16_bits(u: np.ndarray) -> np.ndarray:
    u = np.asarray(u, dtype=np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)).astype(np.uint32)


def q_fixed(x, codes, shared) -> np.ndarray:
    """q_E of the module docstring, elementwise: x float32 (or float64, rounded to float32 first), codes MIXED_TILE_FORMATS codes and
    shared the exponent E (both broadcast) → float32."""
    u = np.ascontiguousarray(np.asarray(x).astype(np.float32)).view(np.uint32)
    c = np.broadcast_to(np.asarray(codes, dtype=np.int64), u.shape)
    out = _bf16_bits(u)
    for code, m in _MANT.items():
        sel = c == code
        if sel.any():
            out = np.where(sel, bfp_fixed_bits(u, shared, m), out)
    return out.view(np.float32)


def group_exponent(x32: np.ndarray) -> np.ndarray:
    """Max exponent field of each row of x32 (float32, [..., g])."""
    return _exp_field(np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)).max(axis=-1)


# ----------------------------------------------------------------------------- margins

def _f64_edge(b32: np.ndarray) -> np.ndarray:
    """The float64 value above which float32 rounding (RNE) reaches the positive float32 b32: b − (gap below b)/2."""
    b = np.asarray(b32, dtype=np.float32)
    prev = (b.view(np.uint32) - np.uint32(1)).view(np.float32)
    return 0.5 * (b.astype(np.float64) + prev.astype(np.float64))


def _level_margin(x: np.ndarray, q: np.ndarray, codes: np.ndarray, shared: np.ndarray) -> np.ndarray:
    """Distance of |x| (float64) to the nearest float64 value that changes its quantisation level, over the element's step."""
    ax = np.abs(x)
    aq = np.abs(q.astype(np.float32))
    out = np.full(x.shape, np.inf)
    # bf16: the grid neighbours of Q and the float32 words where RNE on the low 16 bits moves to them
    Q = aq.view(np.uint32).astype(np.int64)
    ebits = Q & 0x7F800000
    step_bf = (np.where(ebits == 0, 0x00800000, ebits).astype(np.uint32).view(np.float32).astype(np.float64)) * 2.0 ** -7
    up = Q + np.where((Q >> 16) & 1 == 1, 0x8000, 0x8001)
    P = Q - 0x10000
    dn = P + np.where((P >> 16) & 1 == 1, 0x8000, 0x8001)
    m_up = _f64_edge(up.astype(np.uint32).view(np.float32)) - ax
    m_dn = np.where(Q > 0, ax - _f64_edge(np.maximum(dn, 1).astype(np.uint32).view(np.float32)), np.inf)
    out = np.where(codes == 0, np.minimum(m_up, m_dn) / step_bf, out)
    E = np.broadcast_to(np.asarray(shared, dtype=np.int64), x.shape)
    for code, m in _MANT.items():
        sel = codes == code
        if not sel.any():
            continue
        step = np.ldexp(1.0, (E - 126 - m).astype(np.int64))
        t = np.ldexp(1.0, (E - 150).astype(np.int64))
        i = np.rint(aq.astype(np.float64) / step).astype(np.int64)
        qmax = (1 << m) - 1
        # the least float32 |v| of level ≥ i + 1 is (i + ½)·step, one truncation unit t higher for even i (the rule drops the bits
        # below t before its round-half-even)
        b_up = (i + 0.5) * step + np.where(i % 2 == 0, t, 0.0)
        b_dn = (i - 0.5) * step + np.where((i - 1) % 2 == 0, t, 0.0)
        with np.errstate(invalid="ignore"):
            mu = np.where(i < qmax, _f64_edge(b_up.astype(np.float32)) - ax, np.inf)
            md = np.where(i >= 1, ax - _f64_edge(np.maximum(b_dn, np.finfo(np.float32).tiny).astype(np.float32)), np.inf)
        mg = np.minimum(mu, md) / step
        # E = 0: every level is 0 until a value reaches 2^-126 (exponent field 1, saturating); 0 < E ≤ M + 1: the subnormal range
        # cuts into the levels, not modelled — the element counts as undecided
        mg = np.where(E == 0, (_f64_edge(np.float32(2.0 ** -126)) - ax) / step, mg)
        mg = np.where((E > 0) & (E <= m + 1), 0.0, mg)
        out = np.where(sel, mg, out)
    return out


def _exponent_margin(g64: np.ndarray, E: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Distance of the group's largest |value| to the float64 values that change its maximum exponent field E, over the group's
    BFP step (m: mantissa bits per row)."""
    mx = np.abs(g64).max(axis=-1)
    step = np.ldexp(1.0, (E - 126 - m).astype(np.int64))
    with np.errstate(over="ignore", invalid="ignore"):
        hi = _f64_edge(np.ldexp(1.0, (E - 126).astype(np.int64)).astype(np.float32))
        lo = np.where(E > 0, _f64_edge(np.ldexp(1.0, (np.maximum(E, 1) - 127).astype(np.int64)).astype(np.float32)), -np.inf)
    return np.minimum(hi - mx, mx - lo) / step


# ----------------------------------------------------------------------------- Hessian and factorisation

def gram_full_emulation(chunk_iter: Iterable, k: int) -> tuple[np.ndarray, int]:
    """Float64 host route → (H k × k, tokens)."""
    import torch

    h = torch.zeros((k, k), dtype=torch.float64)
    m = 0
    for ch in chunk_iter:
        if ch.x.shape[0] == 0:
            continue
        x = ch.x.to(torch.float64)
        h += x.T @ x
        m += int(x.shape[0])
    return h.numpy(), m


def gram_full_hip(chunk_iter: Iterable, k: int, device=None):
    """mtq_gram_full over every chunk, H carried on the device → (H device tensor k × k float64, tokens)."""
    import torch

    from . import hip_backend as hb

    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    h = torch.zeros((k, k), dtype=torch.float64, device=dev)
    scratch = None
    m = 0
    for ch in chunk_iter:
        if ch.x.shape[0] == 0:
            continue
        xd = ch.x.to(dev).contiguous()
        need = max(hb.gram_full_scratch(int(xd.shape[0]), k), 1)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty((need,), dtype=torch.float64, device=dev)
        hb.gram_full(xd, h, scratch)
        m += int(xd.shape[0])
    return h, m


def damped_hessian(h, damp: float = DEFAULT_DAMP) -> np.ndarray:
    """Steps 2 and 3 of the contract → H_d (float64 k × k)."""
    damp = check_damp(damp)
    hd = np.array(h.cpu().numpy() if hasattr(h, "cpu") else h, dtype=np.float64, copy=True)
    idx = np.arange(hd.shape[0])
    dead = hd[idx, idx] == 0.0
    hd[idx[dead], idx[dead]] = 1.0
    lam = damp * float(np.mean(hd[idx, idx]))
    hd[idx, idx] += lam
    return hd


def factor(h, damp: float = DEFAULT_DAMP) -> Union[np.ndarray, str]:
    """U, the upper Cholesky factor of H_d⁻¹ (float64 k × k, zeros below the diagonal), or the reason there is none."""
    import torch

    hd = torch.from_numpy(damped_hessian(h, damp))
    if not bool(torch.isfinite(hd).all()):
        return "the calibration Hessian holds a non-finite value"
    L, info = torch.linalg.cholesky_ex(hd)
    if int(info) != 0:
        return f"Cholesky factorisation of the damped Hessian failed (leading minor {int(info)})"
    hinv = torch.cholesky_inverse(L)
    U, info = torch.linalg.cholesky_ex(hinv, upper=True)
    if int(info) != 0 or not bool(torch.isfinite(U).all()):
        return "Cholesky factorisation of the inverse damped Hessian failed"
    return U.numpy()


# ----------------------------------------------------------------------------- sweep

def _w32(w) -> np.ndarray:
    return np.asarray(w.float().cpu().numpy() if hasattr(w, "cpu") else w, dtype=np.float32)


def sweep_emulation(w, u, codes, block: int = 128) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The sweep on the host in float64 → (Ŵ float32 n × k, loss float64 [n], margin float64 [n])."""
    w32 = _w32(w)
    n, k = w32.shape
    U = np.asarray(u.cpu().numpy() if hasattr(u, "cpu") else u, dtype=np.float64)
    if U.shape != (k, k):
        raise ValueError(f"u has shape {U.shape}, expected ({k}, {k})")
    U = np.triu(U)
    c = np.asarray(codes, dtype=np.int8)
    if c.shape != (-(-n // TILE), -(-k // TILE)):
        raise ValueError(f"codes has shape {c.shape}, expected {(-(-n // TILE), -(-k // TILE))}")
    if c.size and (c.min() < 0 or c.max() >= len(MIXED_TILE_FORMATS)):
        raise ValueError("codes must be MIXED_TILE_FORMATS codes 0..3")
    crow = np.repeat(c.astype(np.int64), TILE, axis=0)[:n]       # [n, tw]
    W = w32.astype(np.float64)
    q = np.zeros((n, k), dtype=np.float32)
    err = np.zeros((n, k), dtype=np.float64)
    loss = np.zeros(n, dtype=np.float64)
    margin = np.full(n, np.inf)
    E = np.zeros(n, dtype=np.int64)
    mant = np.array([0, 7, 3, 1], dtype=np.int64)
    for b0 in range(0, k, block):
        b1 = min(k, b0 + block)
        for j in range(b0, b1):
            f = crow[:, j // TILE]
            if j % GROUP == 0:
                g = W[:, j: min(k, j + GROUP)]
                E = group_exponent(g.astype(np.float32))
                bfp = f != 0
                if bfp.any():
                    em = _exponent_margin(g[bfp], E[bfp], mant[f[bfp]])
                    margin[bfp] = np.minimum(margin[bfp], em)
            x = W[:, j]
            qj = q_fixed(x, f, E)
            margin = np.minimum(margin, _level_margin(x, qj, f, E))
            e = (x - qj.astype(np.float64)) / U[j, j]
            W[:, j + 1: b1] -= np.outer(e, U[j, j + 1: b1])
            q[:, j] = qj
            err[:, j] = e
            loss += e * e
        if b1 < k:
            W[:, b1:] -= err[:, b0:b1] @ U[b0:b1, b1:]
    return q, loss, margin


def sweep_hip(w, u, codes):
    """mtq_gptq_sweep on the device → (Ŵ float32 device tensor n × k, loss float64 device tensor [n])."""
    import torch

    from . import hip_backend as hb

    wd = w if w.dtype in (torch.bfloat16, torch.float32) else w.float()
    wd = wd if wd.stride(-1) == 1 else wd.contiguous()
    ud = u if hasattr(u, "is_cuda") and u.is_cuda else torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(wd.device)
    cd = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int8)).to(wd.device)
    return hb.gptq_sweep(wd, ud.contiguous(), cd)


def quadratic_loss(w, what, hd) -> np.ndarray:
    """δ_r H_d δ_rᵀ per row, δ = W − Ŵ (float64): the identity Σ_r loss_r must meet."""
    d = _w32(w).astype(np.float64) - np.asarray(what, dtype=np.float64)
    return np.einsum("ra,ab,rb->r", d, np.asarray(hd, dtype=np.float64), d)
