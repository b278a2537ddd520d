"""mixed-tile-budget: the tile map of least weight-space error at a size target (no reference counterpart).

Where the three searches answer "how small at metric >= x", this one answers "N bits per weight, least error": the rule of
budget_maps.allocate (lower convex hull per tile, segments by slope, taken while the size model stays within bits / 8 · 1024 · tiles
bytes) on the table e_w[t, f] = Σ (K2_f(w) − w)² over the tile — the map the layer-output error calls budget:<bits>:weight.

emulation: budget_maps.tile_error_tables_emulation and allocate on the host.  hip: mtq_tile_sq_error_batched and
mtq_budget_allocate_device; only the map, the counts and the status come home, and the status is turned into allocate's reasons.
params: bits (0 < bits <= 16), scope "tensor" (each tensor its own budget; the default) or "model" (one budget over a selection:
pack_model.py), metric (of the reported columns only), formats.  The transposed layout is out of scope and refused.
"""
from __future__ import annotations

import numpy as np

from .. import budget_maps as bm
from .base import CompressionAlgorithm, CompressionResult
from .cache import CacheContext
from .mixed_tile_greedy import parse_tile_formats
from .quantizer import Quantizer
from .tile_search import columns_from_stats, compute_tile_stats, reconstruct
from .tile_utils import MIXED_TILE_BYTES_PER_ELEM, MIXED_TILE_FORMATS, mixed_tile_total_bytes

SCOPES = ("tensor", "model")


def budget_bytes(bits: float, tiles: int) -> float:
    """allocate's budget of `tiles` tiles at `bits` per weight, as it forms it."""
    return float(bits) / 8.0 * float(bm.TILE * bm.TILE) * float(tiles)


def cheapest_format(formats) -> str:
    """The candidate every tile starts at: the least bytes, the lower code on a tie (hull_segments' order)."""
    cands = [f for f in MIXED_TILE_FORMATS if f in set(formats)]
    return min(cands, key=lambda f: (MIXED_TILE_BYTES_PER_ELEM[f], MIXED_TILE_FORMATS.index(f)))


def status_reason(status: int, formats, bits: float, tiles: int):
    """allocate's reason string for a status of mtq_budget_allocate_device (None for 0)."""
    if status == 0:
        return None
    if status == 2:
        return "the tile error table holds a non-finite value"
    if status == 1:
        cheapest = cheapest_format(formats)
        counts = {f: 0 for f in MIXED_TILE_FORMATS}
        counts[cheapest] = int(tiles)
        return (f"budget {budget_bytes(bits, tiles):.0f} B ({bm.bits_tag(bits)} bits) is below the all-{cheapest} size "
                f"{mixed_tile_total_bytes(counts):.0f} B")
    raise ValueError(f"unknown budget status {status}")


def allocate_device(table, formats, bits: float, grid=None):
    """budget_maps.allocate for one device table [T, 4] through mtq_budget_allocate_device → (assignment, counts, tile_bytes) or the
    reason, as allocate returns them."""
    import torch

    from .. import hip_backend as hb

    bits = bm.check_bits(bits)
    T = int(table.shape[0])
    grid = (1, T) if grid is None else tuple(int(v) for v in grid)
    if grid[0] * grid[1] != T:
        raise ValueError(f"grid {grid} does not hold {T} tiles")
    cands = [f for f in MIXED_TILE_FORMATS if f in set(formats)]
    if not cands:
        return f"no mixed-tile format ({', '.join(MIXED_TILE_FORMATS)}) among the candidates"
    first = torch.tensor([0, T], dtype=torch.int64, device=table.device)
    budget = torch.tensor([budget_bytes(bits, T)], dtype=torch.float64, device=table.device)
    maps, counts, status = hb.budget_allocate_device(table, first, cands, budget)
    reason = status_reason(int(status.cpu()[0]), cands, bits, T)
    if reason is not None:
        return reason
    c = counts.cpu().numpy()[0]
    counts_d = {f: int(c[i]) for i, f in enumerate(MIXED_TILE_FORMATS)}
    return maps.cpu().numpy().reshape(grid), counts_d, mixed_tile_total_bytes(counts_d)


class MixedTileBudgetCompression(CompressionAlgorithm):
    name = "mixed-tile-budget"

    def __init__(self, params: dict | None = None) -> None:
        super().__init__(params=params)
        self.metric = self.params.get("metric", "pcc")
        if "bits" not in self.params:
            raise ValueError("mixed-tile-budget needs params.bits (bits per weight, 0 < bits <= 16)")
        self.bits = bm.check_bits(self.params["bits"])
        self.scope = self.params.get("scope", "tensor")
        raw_formats = self.params.get("formats", self.params.get("tile_formats"))
        self.tile_formats = parse_tile_formats(raw_formats) if raw_formats is not None else None
        self.materialize_y = bool(self.params.get("materialize_y", True))
        self.layout = "rows"
        if self.metric not in {"pcc", "mae", "atol"}:
            raise ValueError(f"Unsupported metric: {self.metric}")
        if self.scope not in SCOPES:
            raise ValueError(f"Unsupported scope: {self.scope!r} (expected one of {', '.join(SCOPES)})")
        if self.params.get("layout", "rows") != "rows":
            raise ValueError(f"mixed-tile-budget runs in the row layout only: layout {self.params['layout']!r} is not supported")

    @classmethod
    def from_params(cls, params: dict | None = None) -> "MixedTileBudgetCompression":
        return cls(params=params or {})

    def expected_evals(self, formats: list[str]) -> int:
        return 1

    _parse_formats = staticmethod(parse_tile_formats)

    @staticmethod
    def _filter_from_formats(formats: list[str]) -> list[str]:
        allowed = [fmt for fmt in formats if fmt in MIXED_TILE_FORMATS]
        if not allowed:
            raise ValueError(f"mixed-tile-budget requires at least one of {', '.join(MIXED_TILE_FORMATS)} in quantization_formats")
        return allowed

    def candidates(self, formats: list[str]) -> list[str]:
        return self.tile_formats or self._filter_from_formats(formats)

    def run(self, xf, formats: list[str], quantizer: Quantizer, cache: CacheContext) -> list[CompressionResult]:
        if self.scope == "model":
            raise ValueError("mixed-tile-budget with scope 'model' allocates over a whole selection: run it through scripts/pack_model.py")
        tile_formats = self.candidates(formats)
        size = int(np.asarray(xf).size) if isinstance(xf, np.ndarray) or np.isscalar(xf) else int(xf.numel())
        if size == 0:
            y = np.asarray(xf, dtype=np.float32)
            counts = {fmt: 0 for fmt in MIXED_TILE_FORMATS}
            meta = {"assignment": np.zeros((1, 1), dtype=np.int8), "tile_formats": tile_formats, "bits": self.bits, "budget_bytes": 0.0,
                    "predicted_sse": 0.0}
        else:
            ts = compute_tile_stats(xf, tile_formats, quantizer)
            grid = (ts.tiles_h, ts.tiles_w)
            if ts.backend == "hip":
                from .. import hip_backend as hb

                table_dev = hb.tile_sq_error_batched(ts.x2d)[0]
                got = allocate_device(table_dev, tile_formats, self.bits, grid)
                table = None if isinstance(got, str) else table_dev.cpu().numpy()
            else:
                table = bm.tile_error_tables_emulation(ts.x2d, np.zeros((ts.tiles_w, bm.TILE, bm.TILE)))[1]
                got = bm.allocate(table, tile_formats, self.bits, grid)
            if isinstance(got, str):
                raise ValueError(got)
            assignment, counts, _bytes = got
            y = reconstruct(ts, assignment, quantizer) if self.materialize_y else None
            meta = {"assignment": assignment, "tile_formats": tile_formats, "columns": columns_from_stats(ts, assignment),
                    "bits": self.bits, "budget_bytes": budget_bytes(self.bits, ts.tiles), "predicted_sse": bm.predicted_sse(table, assignment)}
        return [CompressionResult(fmt="MIXED", compression=self.name, y=y, tile_counts=counts, tile_bytes=mixed_tile_total_bytes(counts),
                                  meta=meta)]
