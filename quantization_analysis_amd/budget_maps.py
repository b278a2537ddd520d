"""Activation-aware tile maps under a bit budget, for the layer-output error (output_error.py, scripts/layer_output_error.py).

Inputs: W is one op's weight, n × k (bf16 or float32, nn.Linear convention); X_cal its calibration activations, m × k bf16 as
layer_io.chunks yields them.  The tiles are the 32 × 32 row-layout tiles of W, tiles_hw(n, k), zero padded; c is a tile's column block.

Gram blocks: H_c = X_cal[:, 32c : 32c+32]ᵀ · X_cal[:, 32c : 32c+32], a 32 × 32 float64 block (columns past k are zero), for the
ceil(k/32) column blocks.  Only the diagonal blocks of XᵀX are formed.

Tile error tables: for f in MIXED_TILE_FORMATS, Δ_f = Ŵ_f − W with Ŵ_f = quantize_weight_values(W, f) in the row layout (the Ŵ that K3
and the LOE map slot build for a tile coded f).  For tile t = (r, c), δ_i row i of the tile in Δ_f:
  e_out[t, f] = Σ_i δ_iᵀ H_c δ_i — the tile's share of ‖X_cal·Δᵀ‖²_F when the cross-block terms are dropped;
  e_w[t, f]   = Σ δ² over the tile — the plain weight-space squared error.
Both are float64 [T, 4], indexed by the MIXED_TILE_FORMATS code; a bias cancels in Δ and plays no part.

Allocation (host NumPy, float64, shared by both backends: equal tables give equal maps):
  * candidates: the run's formats ∩ MIXED_TILE_FORMATS; a tile coded f costs 1024 · MIXED_TILE_BYTES_PER_ELEM[f] bytes (padded tiles
    count whole, as in mixed_tile_total_bytes); `bits` in (0, 16] gives a budget of bits / 8 · 1024 · T bytes;
  * every tile starts at the cheapest candidate and walks the lower convex hull of its points (bytes_f, e_f) upward: each step is a
    segment with gain = e_lo − e_hi > 0 and slope gain / Δbytes; of several next points on one slope the cheaper is taken, and a step
    that gains nothing is never made, so equal errors keep the cheaper format;
  * all segments are sorted by (slope descending, tile ascending, step ascending) and taken in that order while
    mixed_tile_total_bytes(counts) stays within the budget, stopping at the first that does not fit.
  The result minimises Σe + λ·bytes for some λ ≥ 0, so no assignment of at most its bytes has a smaller Σe.  No map is made (a reason is
  returned instead) when the budget is below the all-cheapest size, when no candidate is a mixed-tile format, or when a table holds a
  non-finite value.

Two maps per budget, from the same rule: `budget:<bits>:output` allocated on e_out (activation-aware) and `budget:<bits>:weight` on e_w
(the weight-only baseline at the same budget).  The LOE evaluates both exactly, cross terms included, on the evaluation chunks; the
block-diagonal model only chooses the map.

Transposed layout (layout="transpose"; output_error's budget:<bits>:<basis>+transpose): Δ_f = quantize_weight_values(Wᵀ, f)ᵀ − W, whose
groups are 16 consecutive rows of one column, and the tiles are those of Wᵀ's grid, tiles_hw(k, n): tile (r, c) holds columns 32r .. of
W (Wᵀ's rows) and rows 32c .. (Wᵀ's columns).  The same block-diagonal model applies with δ_i row i of W restricted to the tile's column
block r: e_out[t, f] = Σ_i δ_iᵀ H_r δ_i with the same Gram blocks.  allocate is unchanged (grid = tiles_hw(k, n)), and
reconstruct_emulation(w, a, "transpose") is the map's Ŵ, as reconstruct_mixed_tile_assignment.py --layout transpose builds it.

Backends: emulation — float64 torch / NumPy on the host; hip — csrc/mtq_budget.hip (mtq_gram_blocks per chunk, then
mtq_tile_error_tables or mtq_tile_error_tables_transposed and one device-to-host copy).

The mixed-tile-budget algorithm (compression_algorithms/mixed_tile_budget.py) applies the same rule to e_w alone, per tensor or — scope
"model", model_maps below — with one budget over the concatenated tables of a selection.  Its hip route allocates on the device
(mtq_budget_allocate_device) under the contract that map and counts equal allocate's for every finite table: allocate is the oracle.
"""
from __future__ import annotations

from typing import Iterable, Optional, Union

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_BYTES_PER_ELEM, MIXED_TILE_FORMATS, mixed_tile_total_bytes
from .quantization_formats import quantize_weight_values

TILE = 32
BASES = ("output", "weight")


def tiles_hw(n: int, k: int) -> tuple[int, int]:
    return -(-n // TILE), -(-k // TILE)


def check_bits(bits: float) -> float:
    b = float(bits)
    if not (0.0 < b <= 16.0):
        raise ValueError(f"bits per weight must be in (0, 16], got {bits!r}")
    return b


def bits_tag(bits: float) -> str:
    """4.0 → '4', 4.5 → '4.5': the <bits> of the map names and of the saved files."""
    return format(float(bits), "g")


def map_name(bits: float, basis: str) -> str:
    return f"budget:{bits_tag(bits)}:{basis}"


# ----------------------------------------------------------------------------- Gram blocks

def gram_blocks_emulation(chunk_iter: Iterable, k: int) -> tuple[np.ndarray, int]:
    """Float64 host route → (H [ceil(k/32), 32, 32], tokens)."""
    import torch

    nb = -(-k // TILE)
    h = torch.zeros((nb, TILE, TILE), dtype=torch.float64)
    m = 0
    for ch in chunk_iter:
        x = ch.x.to(torch.float64)
        if x.shape[0] == 0:
            continue
        xp = torch.zeros((x.shape[0], nb * TILE), dtype=torch.float64)
        xp[:, :k] = x
        xb = xp.view(x.shape[0], nb, TILE)
        h += torch.einsum("mbi,mbj->bij", xb, xb)
        m += int(x.shape[0])
    return h.numpy(), m


def gram_blocks_hip(chunk_iter: Iterable, k: int, device=None):
    """mtq_gram_blocks over every chunk, H carried on the device → (H device tensor [ceil(k/32), 32, 32], tokens)."""
    import torch

    from . import hip_backend as hb

    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    h = torch.zeros((-(-k // TILE), TILE, TILE), dtype=torch.float64, device=dev)
    scratch = None
    m = 0
    for ch in chunk_iter:
        if ch.x.shape[0] == 0:
            continue
        xd = ch.x.to(dev).contiguous()
        need = hb.gram_blocks_scratch(int(xd.shape[0]), k)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty((need,), dtype=torch.float64, device=dev)
        hb.gram_blocks(xd, h, scratch)
        m += int(xd.shape[0])
    return h, m


# ----------------------------------------------------------------------------- tile error tables

def _w32(w) -> np.ndarray:
    return np.asarray(w.float().cpu().numpy() if hasattr(w, "cpu") else w, dtype=np.float32)


def tile_error_tables_emulation(w, h, layout: str = "rows") -> tuple[np.ndarray, np.ndarray]:
    """Float64 host route → (e_out, e_w), each [T, 4].  w: (n, k) weight (torch or NumPy); h: [ceil(k/32), 32, 32] Gram blocks.
    layout "transpose": Δ from column groups, tiles over Wᵀ's grid (module docstring)."""
    w32 = _w32(w)
    n, k = w32.shape
    th, tw = tiles_hw(n, k)
    h = np.asarray(h.cpu().numpy() if hasattr(h, "cpu") else h, dtype=np.float64)
    if h.shape != (tw, TILE, TILE):
        raise ValueError(f"h has shape {h.shape}, expected ({tw}, 32, 32)")
    w64 = w32.astype(np.float64)
    e_out = np.zeros((th * tw, len(MIXED_TILE_FORMATS)), dtype=np.float64)
    e_w = np.zeros_like(e_out)
    if layout == "transpose":
        wt = np.ascontiguousarray(w32.T)
        for code, f in enumerate(MIXED_TILE_FORMATS):
            d = np.zeros((tw * TILE, th * TILE), dtype=np.float64)             # Δᵀ over Wᵀ's grid
            d[:k, :n] = quantize_weight_values(wt, f).astype(np.float64) - w64.T
            dt = d.reshape(tw, TILE, th, TILE)                                 # [r, a, c, i]: column a of W's block r, row i
            g = np.einsum("raci,rab->rbci", dt, h)                             # (H_r δ_i)[b]
            e_out[:, code] = np.einsum("rbci,rbci->rc", g, dt).reshape(-1)
            e_w[:, code] = np.einsum("raci,raci->rc", dt, dt).reshape(-1)
        return e_out, e_w
    if layout != "rows":
        raise ValueError(f"layout must be rows or transpose, got {layout!r}")
    for code, f in enumerate(MIXED_TILE_FORMATS):
        d = np.zeros((th * TILE, tw * TILE), dtype=np.float64)
        d[:n, :k] = quantize_weight_values(w32, f).astype(np.float64) - w64
        dt = d.reshape(th, TILE, tw, TILE)                                   # [r, i, c, a]
        g = np.einsum("rica,cab->ricb", dt, h)                               # δ_iᵀ H_c
        e_out[:, code] = np.einsum("ricb,ricb->rc", g, dt).reshape(-1)
        e_w[:, code] = np.einsum("rica,rica->rc", dt, dt).reshape(-1)
    return e_out, e_w


def tile_error_tables_hip(w, h, layout: str = "rows") -> tuple[np.ndarray, np.ndarray]:
    """mtq_tile_error_tables (layout "transpose": mtq_tile_error_tables_transposed) on the device weight and Gram blocks, then one
    device-to-host copy → (e_out, e_w), each [T, 4]."""
    import torch

    from . import hip_backend as hb

    wd = w if w.dtype in (torch.bfloat16, torch.float32) else w.float()
    wd = wd if wd.stride(-1) == 1 else wd.contiguous()
    if layout not in ("rows", "transpose"):
        raise ValueError(f"layout must be rows or transpose, got {layout!r}")
    fn = hb.tile_error_tables_transposed if layout == "transpose" else hb.tile_error_tables
    e_out, e_w = fn(wd, h, want_weight=True)
    both = torch.stack((e_out, e_w)).cpu().numpy()
    return both[0], both[1]


# ----------------------------------------------------------------------------- allocation

def hull_segments(e: np.ndarray, cands) -> tuple:
    """The segments of every tile's lower convex hull, in the order the allocation takes them → (order, tile, from, to, slope): order
    = the candidates by ascending bytes, from / to index into it; slope = the sort key (gain / Δbytes, clamped so that a tile's steps
    stay in order even where rounding lifts a later slope)."""
    cost = {f: float(TILE * TILE) * MIXED_TILE_BYTES_PER_ELEM[f] for f in cands}
    order = sorted(cands, key=lambda f: (cost[f], MIXED_TILE_FORMATS.index(f)))
    T = int(e.shape[0])
    pts_b = np.array([cost[f] for f in order])
    pts_e = e[:, [MIXED_TILE_FORMATS.index(f) for f in order]]
    P = len(order)
    cur = np.zeros(T, dtype=np.int64)
    key_prev = np.full(T, np.inf)
    segs = []
    tiles = np.arange(T)
    for step in range(P - 1):                                  # each step moves to a strictly dearer point
        e_cur = pts_e[tiles, cur]
        b_cur = pts_b[cur]
        best = np.full(T, -np.inf)
        nxt = np.full(T, -1, dtype=np.int64)
        for q in range(P):                                     # ascending bytes: a strict > keeps the cheaper point on a tie
            gain = e_cur - pts_e[:, q]
            db = pts_b[q] - b_cur
            ok = (db > 0) & (gain > 0)
            slope = np.where(ok, gain / np.where(db > 0, db, 1.0), -np.inf)
            better = ok & (slope > best)
            best = np.where(better, slope, best)
            nxt = np.where(better, q, nxt)
        live = nxt >= 0
        if not live.any():
            break
        key = np.minimum(best, key_prev)
        idx = np.nonzero(live)[0]
        segs.append((idx, np.full(idx.size, step), key[idx], cur[idx].copy(), nxt[idx]))
        key_prev = np.where(live, key, key_prev)
        cur = np.where(live, nxt, cur)
    if not segs:
        z = np.zeros(0, dtype=np.int64)
        return order, z, z, z, np.zeros(0)
    st, ss, sk, sf, sto = (np.concatenate(v) for v in zip(*segs))
    srt = np.lexsort((ss, st, -sk))                            # slope descending, tile ascending, step ascending
    return order, st[srt], sf[srt], sto[srt], sk[srt]


def allocate(table: np.ndarray, formats, bits: float, grid: Optional[tuple] = None) -> Union[tuple, str]:
    """The map of least Σ table under the budget (the rule of the module docstring) → (assignment int8 [th, tw], counts, tile_bytes),
    or the reason no map is made.  table: float64 [T, 4] by MIXED_TILE_FORMATS code; grid: (th, tw) with th · tw = T (default (1, T))."""
    bits = check_bits(bits)
    e = np.asarray(table, dtype=np.float64)
    if e.ndim != 2 or e.shape[1] != len(MIXED_TILE_FORMATS):
        raise ValueError(f"table must be [tiles, {len(MIXED_TILE_FORMATS)}], got {e.shape}")
    T = int(e.shape[0])
    grid = (1, T) if grid is None else tuple(int(v) for v in grid)
    if grid[0] * grid[1] != T:
        raise ValueError(f"grid {grid} does not hold {T} tiles")
    cands = [f for f in MIXED_TILE_FORMATS if f in set(formats)]
    if not cands:
        return f"no mixed-tile format ({', '.join(MIXED_TILE_FORMATS)}) among the candidates"
    if not np.all(np.isfinite(e)):
        return "the tile error table holds a non-finite value"
    order, tiles, frm, to, _slope = hull_segments(e, cands)
    cheapest = order[0]
    budget = bits / 8.0 * float(TILE * TILE) * float(T)
    counts = {f: 0 for f in MIXED_TILE_FORMATS}
    counts[cheapest] = T
    floor = mixed_tile_total_bytes(counts)
    if floor > budget:
        return f"budget {budget:.0f} B ({bits_tag(bits)} bits) is below the all-{cheapest} size {floor:.0f} B"
    # counts after every prefix of the sorted segments, and mixed_tile_total_bytes of each with its accumulation order
    cnt = {f: (T if i == 0 else 0) + np.cumsum((to == i).astype(np.int64) - (frm == i).astype(np.int64)) for i, f in enumerate(order)}
    total = np.zeros(tiles.size, dtype=np.float64)
    for f in MIXED_TILE_FORMATS:                               # formats outside the candidates add +0.0
        if f in cnt:
            total = total + (cnt[f].astype(np.float64) * float(TILE * TILE)) * MIXED_TILE_BYTES_PER_ELEM[f]
    over = np.nonzero(total > budget)[0]
    take = int(over[0]) if over.size else int(tiles.size)
    # the segments a tile has taken are its first hull steps, each to a dearer point: its final point is the dearest
    assign_idx = np.zeros(T, dtype=np.int64)
    np.maximum.at(assign_idx, tiles[:take], to[:take])
    codes = np.array([MIXED_TILE_FORMATS.index(f) for f in order])
    assignment = codes[assign_idx].astype(np.int8).reshape(grid)
    counts = {f: int(np.count_nonzero(assignment == c)) for c, f in enumerate(MIXED_TILE_FORMATS)}
    return assignment, counts, mixed_tile_total_bytes(counts)


def model_budget(bits: float, tiles: int) -> float:
    """allocate's budget for `tiles` tiles in all: bits / 8 · 1024 · tiles bytes."""
    return check_bits(bits) / 8.0 * float(TILE * TILE) * float(tiles)


def split_maps(flat_map, grids) -> list:
    """One map over the tiles of several tensors numbered through, tensor j's th_j · tw_j tiles behind tensor j−1's → the tensors' own
    int8 [th_j, tw_j] maps."""
    flat = np.asarray(flat_map, dtype=np.int8).reshape(-1)
    sizes = [int(th) * int(tw) for th, tw in grids]
    if sum(sizes) != flat.size:
        raise ValueError(f"the grids hold {sum(sizes)} tiles, the map {flat.size}")
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return [flat[first[j]:first[j + 1]].reshape(g) for j, g in enumerate(grids)]


def model_maps(tables, grids, formats, bits: float) -> Union[tuple, str]:
    """One budget over a whole selection (scope "model"): the tensors' tables [T_j, 4] are concatenated in order, tiles numbered
    through, and allocate runs once with bits / 8 · 1024 · Σ T_j bytes, so a sensitive tensor takes bytes from an insensitive one →
    (maps: each tensor's int8 [th_j, tw_j], counts over everything, tile_bytes), or allocate's reason."""
    table = np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1, len(MIXED_TILE_FORMATS)) for t in tables])
    got = allocate(table, formats, bits)
    if isinstance(got, str):
        return got
    return split_maps(got[0], grids), got[1], got[2]


def predicted_sse(table: np.ndarray, assignment: np.ndarray) -> float:
    """Σ_t table[t, assignment_t] (float64, tile order)."""
    a = np.asarray(assignment, dtype=np.int64).reshape(-1)
    return float(np.asarray(table, dtype=np.float64)[np.arange(a.size), a].sum())


def reconstruct_emulation(w, assignment: np.ndarray, layout: str = "rows") -> np.ndarray:
    """Ŵ of a map on the host (float32): each tile quantised in the format its entry names, as K3 builds it.  layout "transpose": the
    map is over Wᵀ's grid and Ŵ = (the map's Ŵ of Wᵀ)ᵀ."""
    w32 = _w32(w)
    if layout == "transpose":
        return np.ascontiguousarray(reconstruct_emulation(np.ascontiguousarray(w32.T), assignment).T)
    if layout != "rows":
        raise ValueError(f"layout must be rows or transpose, got {layout!r}")
    n, k = w32.shape
    a = np.asarray(assignment, dtype=np.int8)
    codes = np.repeat(np.repeat(a, TILE, axis=0), TILE, axis=1)[:n, :k]
    y = np.zeros_like(w32)
    for c, f in enumerate(MIXED_TILE_FORMATS):
        sel = codes == c
        if sel.any():
            y[sel] = quantize_weight_values(w32, f)[sel]
    return y
