"""AWQ for BFP: per-input-channel power-of-two scales searched on calibration activations (output_error.py, scripts/layer_output_error.py).

With s_j = 2^p_j, W·2^p is exact in float32 and x·2^−p exact in bf16, so the scaled layer is the original layer bit for bit; what moves is
how the 16 channels of a shared-exponent group split the group's mantissa bits.  A salient input channel shifted up by p keeps p more
bits; its neighbours pay when it lifts the group's exponent.

Inputs: W is n × k (bf16 or float32, nn.Linear convention); `codes` int8 [ceil(n/32), ceil(k/32)] over MIXED_TILE_FORMATS (a pure format
is the constant map, gptq.constant_codes); calibration chunks of X are m × k bf16.  Row layout only: a group is 16 consecutive columns
of one row, a ragged last group holds the columns < k.

Channel statistic (host, float64, shared by both backends): a_j = sqrt(H_jj / m) from the diagonal of the 32 × 32 Gram blocks of
budget_maps.gram_blocks_* (no new pass over X), t_j = log2(a_j).  A dead channel (H_jj == 0) gets the smallest live t; with no live
channel no candidate is made and a reason is returned.

Exponent table (host, shared): α_g = g / G for g = 0 .. G − 1 (G = 20 by default) and
    p[g, j] = min(P, rint(α_g · (t_j − min of t over j's 16-group)))      (np.rint; P = 7 by default, 1 .. 7)
so every group's smallest shift is 0 (a constant added to a whole group changes nothing), row 0 is all zeros (plain RTN), and duplicate
rows are dropped keeping the smallest α: p is int8 [G′, k].

Quantiser, for row r, group c, slot g: E = the maximum over the group's elements with a non-zero float32 exponent field e_i of
e_i + p[g, i] (0 if there are none), and Ŵ_g[r, j] = q_{E − p[g, j]}(w_rj, f) with q_E the fixed-exponent element rule of gptq.py
(q_fixed) and f the code of j's tile.  Saturation never fires (E − p_j ≥ e_j); an element with exponent field 0 gives +0 whatever
E − p_j is; a bf16 tile ignores p.  This equals ldexp(quantize_weight_values(ldexp(W, p), f), −p) wherever every non-zero value's
exponent field stays in [8, 240]; W with an exponent field above 240 is refused on the host with a reason.  Every Ŵ_g has at most 8
significant bits, so it is exact in bf16.

Loss: loss[g] = Σ_{m,n} (fl32(r − q_g))² in float64 over all calibration tokens, r formed exactly as mtq_output_error forms R (the hi /
mid / lo split for float32 W) and q_g = X·Ŵ_gᵀ with exact bf16 products and float32 accumulation.  A bias cancels and is not an
argument; X is never scaled in the search.  The host oracle is Σ (x64 @ (w64 − ŵ64)ᵀ)².

Choice: g* = the smallest g with the least loss; loss[0] is RTN's, so the choice never loses to RTN on the calibration split.  A
non-finite loss vector makes no candidate and returns a reason.

Transposed layout: a per-input-channel shift moves all 16 rows of a column group together and changes nothing, so there is no
transposed candidate.

Deployment: packed.pack(scale_weight(w, p_row), codes) is the deployed weight (plain BFP of the scaled weight, no new byte format) and
PackedLinear / PackedMatmul(in_exponents=p_row) apply torch.ldexp(x, −p) in front of the product (a torch op, not a kernel).

Backends: emulation — NumPy / torch float64 on the host, the oracle of the GPU tests; hip — csrc/mtq_awq.hip (mtq_awq_losses per
chunk with the loss vector carried on the device, mtq_awq_quantize for Ŵ of the chosen row).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional, Union

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from .gptq import GROUP, TILE, _exp_field, _w32, q_fixed

AWQ_FORMATS = ("bfp8", "bfp4", "bfp2")
DEFAULT_GRID = 20
DEFAULT_MAX_SHIFT = 7
MAX_EXP_FIELD = 240


@dataclass
class AwqResult:
    p_row: np.ndarray          # int8 [k], the chosen shifts
    g: int                     # its row in the de-duplicated table
    alpha: float
    losses: np.ndarray         # float64 [G′]; losses[0] is RTN's


def check_params(grid, max_shift) -> tuple[int, int]:
    g, p = int(grid), int(max_shift)
    if g != grid or g < 1:
        raise ValueError(f"grid must be an integer >= 1, got {grid!r}")
    if p != max_shift or not 1 <= p <= 7:
        raise ValueError(f"max_shift must be an integer in 1 .. 7, got {max_shift!r}")
    return g, p


def check_weight(w) -> Optional[str]:
    """The reason W cannot be searched, or None."""
    e = _exp_field(np.ascontiguousarray(_w32(w)).view(np.uint32))
    if e.size and int(e.max()) > MAX_EXP_FIELD:
        return f"the weight holds an exponent field above {MAX_EXP_FIELD} (non-finite or huge values): a shift could overflow"
    return None


def _check_codes(codes, n: int, k: int) -> np.ndarray:
    c = np.asarray(codes, dtype=np.int8)
    if c.shape != (-(-n // TILE), -(-k // TILE)):
        raise ValueError(f"codes has shape {c.shape}, expected {(-(-n // TILE), -(-k // TILE))}")
    if c.size and (c.min() < 0 or c.max() >= len(MIXED_TILE_FORMATS)):
        raise ValueError("codes must be MIXED_TILE_FORMATS codes 0..3")
    return c


def _check_shifts(p, k: int, rank: int) -> np.ndarray:
    a = np.asarray(p)
    if a.ndim != rank or a.shape[-1] != k or (rank == 2 and a.shape[0] < 1):
        raise ValueError(f"the shifts have shape {a.shape}, expected {'(k,)' if rank == 1 else '(G >= 1, k)'} with k = {k}")
    if a.size and (a.min() < 0 or a.max() > 7 or not np.array_equal(a, np.rint(a))):
        raise ValueError("the shifts must be integers in 0 .. 7")
    return np.ascontiguousarray(a, dtype=np.int8)


def channel_log2(h_blocks, m: int) -> Union[np.ndarray, str]:
    """t_j of the contract from the Gram blocks (ceil(k/32), 32, 32) and the token count, over all 32·ceil(k/32) columns (the caller cuts
    to k), or the reason there is none."""
    h = np.asarray(h_blocks.cpu().numpy() if hasattr(h_blocks, "cpu") else h_blocks, dtype=np.float64)
    d = np.einsum("bii->bi", h).reshape(-1)
    if m <= 0:
        return "the calibration samples hold no tokens"
    if not np.isfinite(d).all():
        return "the calibration Gram diagonal holds a non-finite value"
    live = d > 0.0
    if not live.any():
        return "every input channel is dead on the calibration samples"
    t = np.full(d.shape, np.inf)
    t[live] = np.log2(np.sqrt(d[live] / float(m)))
    t[~live] = t[live].min()
    return t


def exponent_table(t, grid: int = DEFAULT_GRID, max_shift: int = DEFAULT_MAX_SHIFT) -> tuple[np.ndarray, np.ndarray]:
    """(alphas float64 [G′], p int8 [G′, k]) of the contract from t [k]."""
    grid, max_shift = check_params(grid, max_shift)
    t = np.asarray(t, dtype=np.float64)
    k = t.shape[0]
    pad = np.full(-(-k // GROUP) * GROUP, np.inf)
    pad[:k] = t
    rel = (pad.reshape(-1, GROUP) - pad.reshape(-1, GROUP).min(axis=1, keepdims=True)).reshape(-1)[:k]
    alphas, rows = [], []
    for g in range(grid):
        a = g / grid
        row = np.minimum(float(max_shift), np.rint(a * rel)).astype(np.int8)
        if not any(np.array_equal(row, r) for r in rows):
            alphas.append(a)
            rows.append(row)
    return np.asarray(alphas, dtype=np.float64), np.stack(rows)


def scale_weight(w, p_row):
    """W·2^p per input channel (float32; torch tensor in, torch tensor out, otherwise NumPy), refusing an overflow."""
    if hasattr(w, "cpu"):
        import torch

        p = torch.from_numpy(_check_shifts(p_row.cpu().numpy() if hasattr(p_row, "cpu") else p_row, int(w.shape[-1]), 1).astype(np.int32)).to(w.device)
        out = torch.ldexp(w.float(), p)
        bad = bool((~torch.isfinite(out) & torch.isfinite(w.float())).any())
    else:
        w32 = np.asarray(w, dtype=np.float32)
        with np.errstate(over="ignore"):
            out = np.ldexp(w32, _check_shifts(p_row, w32.shape[-1], 1).astype(np.int32)).astype(np.float32)
        bad = bool((~np.isfinite(out) & np.isfinite(w32)).any())
    if bad:
        raise ValueError("scaling the weight by its shifts overflows float32")
    return out


# ----------------------------------------------------------------------------- quantiser

def quantize_emulation(w, codes, p_row) -> np.ndarray:
    """Ŵ of one shift row on the host, the oracle of mtq_awq_quantize → float32 n × k."""
    w32 = _w32(w)
    n, k = w32.shape
    c = _check_codes(codes, n, k)
    p = _check_shifts(p_row, k, 1).astype(np.int64)
    kp = -(-k // GROUP) * GROUP
    wp = np.zeros((n, kp), dtype=np.float32)
    wp[:, :k] = w32
    pp = np.zeros(kp, dtype=np.int64)
    pp[:k] = p
    e = _exp_field(wp.view(np.uint32))
    E = np.where(e != 0, e + pp, 0).reshape(n, kp // GROUP, GROUP).max(axis=-1)
    shared = np.where(e != 0, np.repeat(E, GROUP, axis=1) - pp, 0)        # exponent field 0: +0 whatever E − p is (q_fixed would saturate)
    cel = np.repeat(np.repeat(c.astype(np.int64), TILE, axis=0)[:n], TILE, axis=1)[:, :k]
    return q_fixed(wp[:, :k], cel, shared[:, :k])


def _device_operands(w, codes, p, device=None):
    import torch

    dev = device if device is not None else (w.device if hasattr(w, "is_cuda") and w.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    wd = w if hasattr(w, "cpu") else torch.from_numpy(np.asarray(w, dtype=np.float32))
    wd = (wd if wd.dtype in (torch.bfloat16, torch.float32) else wd.float()).to(dev)
    wd = wd if wd.stride(-1) == 1 else wd.contiguous()
    cd = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int8)).to(dev)
    pd = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int8)).to(dev)
    return wd, cd, pd


def quantize_hip(w, codes, p_row):
    """mtq_awq_quantize on the device → Ŵ as a float32 device tensor n × k."""
    from . import hip_backend as hb

    return hb.awq_quantize(*_device_operands(w, codes, p_row))


# ----------------------------------------------------------------------------- losses

def losses_emulation(chunk_iter: Iterable, w, codes, p) -> tuple[np.ndarray, int]:
    """The float64 host oracle → (loss [G′], tokens)."""
    import torch

    w32 = _w32(w)
    p = _check_shifts(p, w32.shape[1], 2)
    deltas = [torch.from_numpy(w32.astype(np.float64) - quantize_emulation(w32, codes, row).astype(np.float64)) for row in p]
    loss = np.zeros(len(deltas), dtype=np.float64)
    m = 0
    for ch in chunk_iter:
        if ch.x.shape[0] == 0:
            continue
        x64 = ch.x.to(torch.float64).cpu()
        for g, d in enumerate(deltas):
            y = x64 @ d.T
            loss[g] += float((y * y).sum())
        m += int(ch.x.shape[0])
    return loss, m


def losses_hip(chunk_iter: Iterable, w, codes, p, device=None):
    """mtq_awq_losses over every chunk, the loss vector carried on the device → (loss float64 device tensor [G′], tokens)."""
    import torch

    from . import hip_backend as hb

    wd, cd, pd = _device_operands(w, codes, _check_shifts(p, int(w.shape[1]), 2), device)
    loss = torch.zeros((pd.shape[0],), dtype=torch.float64, device=wd.device)
    hb.awq_check_values(wd, cd, pd)                                    # once, not per chunk
    scratch = None
    m = 0
    for ch in chunk_iter:
        if ch.x.shape[0] == 0:
            continue
        xd = ch.x.to(wd.device).contiguous()
        need = max(hb.awq_losses_scratch(int(xd.shape[0]), int(wd.shape[0]), int(pd.shape[0])), 1)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty((need,), dtype=torch.float64, device=wd.device)
        hb.awq_losses(xd, wd, cd, pd, loss, scratch, checked=True)
        m += int(xd.shape[0])
    return loss, m


def search(chunk_iter: Iterable, w, codes, h_blocks, m: int, backend: str = "emulation", grid: int = DEFAULT_GRID,
           max_shift: int = DEFAULT_MAX_SHIFT) -> Union[AwqResult, str]:
    """The whole search → AwqResult, or the reason no candidate is made.  h_blocks, m: the Gram blocks and token count of the
    calibration samples (budget_maps.gram_blocks_*); chunk_iter: the same samples again, for the losses."""
    check_params(grid, max_shift)
    if backend not in ("emulation", "hip"):
        raise ValueError("backend must be emulation or hip")
    n, k = int(w.shape[0]), int(w.shape[1])
    _check_codes(codes, n, k)
    why = check_weight(w)
    if why is not None:
        return why
    t = channel_log2(h_blocks, m)
    if isinstance(t, str):
        return t
    alphas, p = exponent_table(t[:k], grid, max_shift)
    if backend == "hip":
        loss, _m = losses_hip(chunk_iter, w, codes, p)
        loss = loss.cpu().numpy()
    else:
        loss, _m = losses_emulation(chunk_iter, w, codes, p)
    if not np.isfinite(loss).all():
        return "the calibration losses hold a non-finite value"
    g = int(np.argmin(loss))                                           # the first of equal minima
    return AwqResult(p_row=p[g].copy(), g=g, alpha=float(alphas[g]), losses=loss)
