"""BudgetPipeline — mixed-tile-budget with the table, the allocation and the records on the device (see pipeline.py for the overview)."""
from __future__ import annotations

import numpy as np

from . import hip_backend as hb
from .compression_algorithms import mixed_tile_budget as mtb
from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS, mixed_tile_total_bytes
from .pipeline_common import TensorResult, columns_from_sums_batch, gated_columns


class BudgetPipeline:
    """mixed-tile-budget (scope "tensor") over a (count, rows, cols) device tensor of equally shaped matrices: K1 (batched) for the
    reported columns → the weight-space error table of every tile in one launch (mtq_tile_sq_error_batched) → ONE allocator call with a
    segment and a budget per tensor (mtq_budget_allocate_device) → the column sums under the device maps.  Nothing is read back between
    the launches; afterwards the status comes home first (a refused tensor raises allocate's reason), then 11 doubles per tensor, the
    counts and the maps (1 B per tile, for the results' assignment).  The maps of the last batch stay available on the device
    (`maps_dev`, int8 [count, tiles]) so that packed.pack_batch takes them without a trip.

    Maps decided elsewhere may be given (`run(x3d, maps=...)`): pack_model's model scope allocates once over every tensor's table
    (`tables`) and then asks only for the columns under its maps."""

    def __init__(self, tile_formats=None, metric: str = "pcc", bits: float = 4.5, chunk: int = 16, pure_formats=()):
        import torch

        hb.require_gpu()
        self.torch = torch
        self.tile_formats = [f for f in MIXED_TILE_FORMATS if f in set(tile_formats or MIXED_TILE_FORMATS)]
        if not self.tile_formats:
            raise ValueError(f"mixed-tile-budget requires at least one of {', '.join(MIXED_TILE_FORMATS)}")
        if metric not in ("pcc", "mae", "atol"):
            raise ValueError(f"Unsupported metric: {metric}")
        self.pure_formats = [f for f in pure_formats if f in self.tile_formats]
        self.mask = hb.fmt_mask(self.tile_formats)
        self.metric, self.bits = metric, mtb.bm.check_bits(bits)
        self.chunk = int(chunk)          # kept for the drivers that set it: a batch is always one launch chain here
        self.maps_dev = None
        self.table_dev = None
        self._scratch_n = hb.columns_scratch_doubles()
        self._pin = {}
        self._dev = {}

    def close(self) -> None:
        """Drains the device and releases the pinned mirrors and the device buffers now."""
        self.torch.cuda.synchronize()
        self._pin.clear()
        self._dev.clear()
        self.maps_dev = self.table_dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _devbuf(self, name: str, numel: int, dtype, device):
        t = self._dev.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype or t.device != device:
            t = self.torch.empty((int(numel * 1.25) + 16,), dtype=dtype, device=device)
            self._dev[name] = t
        return t[:numel]

    def _pinned(self, name: str, numel: int, dtype):
        t = self._pin.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = self.torch.zeros((int(numel * 1.25) + 16,), dtype=dtype, pin_memory=True)
            self._pin[name] = t
        return t[:numel]

    def tables(self, x3d):
        """The weight-space error tables of a batch on the device → float64 [count, tiles, 4] (a fresh tensor: the caller may keep it)."""
        return hb.tile_sq_error_batched(x3d)

    def enqueue(self, x3d, numel: int | None = None, slot: int = 0, maps=None) -> dict:
        """GPU half of a batch, nothing waited for and nothing read back.  maps: int8 device maps [count · tiles] decided elsewhere (the
        model scope) — the table and the allocation are then skipped."""
        torch = self.torch
        count, rows, cols = x3d.shape
        dev = x3d.device
        th, tw = hb.tiles_hw(rows, cols)
        tiles, numel = th * tw, (rows * cols if numel is None else int(numel))
        P = 1 + len(self.pure_formats)
        rec = hb.record_doubles(self.mask)
        recs = self._devbuf(f"recs{slot}", count * tiles * rec, torch.float64, dev).view(count, tiles, rec)
        hb.tile_stats_batched(x3d.contiguous(), self.mask, out=recs)
        counts = status = None
        if maps is None:
            table = self._devbuf(f"table{slot}", count * tiles * 4, torch.float64, dev).view(count, tiles, 4)
            hb.tile_sq_error_batched(x3d, out=table)
            first = torch.arange(0, (count + 1) * tiles, tiles, dtype=torch.int64, device=dev)
            budget = torch.full((count,), mtb.budget_bytes(self.bits, tiles), dtype=torch.float64, device=dev)
            scratch = self._devbuf(f"alloc{slot}", hb.budget_allocate_scratch_bytes(count * tiles, count), torch.uint8, dev)
            maps, counts, status = hb.budget_allocate_device(table.view(count * tiles, 4), first, self.tile_formats, budget, scratch)
            self.table_dev = table
        maps = maps.reshape(count * tiles)
        self.maps_dev = maps.view(count, tiles)
        sums_host = self._pinned(f"sums{slot}", P * count * 11, torch.float64).view(P, count, 11)
        colscr = self._devbuf(f"colscr{slot}", P * count * self._scratch_n, torch.float64, dev).view(P, count, self._scratch_n)
        cur = torch.cuda.current_stream()
        hb.threshold_columns(recs, count, tiles, self.mask, maps, colscr[0], sums_host[0], cur)
        for q, f in enumerate(self.pure_formats):   # wq's `none` rows from the same records
            pure = torch.full((count * tiles,), MIXED_TILE_FORMATS.index(f), dtype=torch.int8, device=dev)
            hb.threshold_columns(recs, count, tiles, self.mask, pure, colscr[1 + q], sums_host[1 + q], cur)
        return {"x": x3d, "numel": numel, "hw": (th, tw), "tiles": tiles, "count": count, "maps": maps, "counts": counts, "status": status,
                "sums_host": sums_host}

    def finish(self, st: dict) -> list[TensorResult]:
        """Host half: the status first, on its own (a refused tensor raises allocate's reason and nothing else is fetched), then the
        sums (behind a wait for the stream), the counts and the maps."""
        count, tiles, (th, tw) = st["count"], st["tiles"], st["hw"]
        if st["status"] is not None:
            status = st["status"].cpu().numpy()
            for j in np.flatnonzero(status):
                raise ValueError(f"tensor {int(j)} of the batch: {mtb.status_reason(int(status[j]), self.tile_formats, self.bits, tiles)}")
        self.torch.cuda.current_stream().synchronize()
        sums = st["sums_host"].numpy()
        maps_all = st["maps"].cpu().numpy().reshape(count, tiles)
        xs, numel = st["x"], float(st["numel"])
        k = {"pcc": 0, "mae": 1, "atol": 2}[self.metric]
        cols = gated_columns(columns_from_sums_batch(sums[0], numel), sums[0], numel, xs,
                             lambda j: hb.apply_assignment(xs[j], maps_all[j].reshape(th, tw)))
        pure_cols = [gated_columns(columns_from_sums_batch(sums[1 + i], numel), sums[1 + i], numel, xs,
                                   lambda j, c=MIXED_TILE_FORMATS.index(f): hb.apply_assignment(xs[j], np.full((th, tw), c, dtype=np.int8)))
                     for i, f in enumerate(self.pure_formats)]
        alloc_counts = None if st["counts"] is None else st["counts"].cpu().numpy()
        results = []
        for j in range(count):
            counts = {f: int(sums[0][j, 7 + i]) for i, f in enumerate(MIXED_TILE_FORMATS)}   # the column kernel's histogram of the map
            if alloc_counts is not None and [counts[f] for f in MIXED_TILE_FORMATS] != alloc_counts[j].tolist():
                raise hb.MtqError(f"tensor {j}: the allocator's counts {alloc_counts[j].tolist()} are not its map's {counts}")
            pure = {f: tuple(float(v) for v in pure_cols[i][j]) for i, f in enumerate(self.pure_formats)} or None
            results.append(TensorResult(j, maps_all[j].reshape(th, tw), counts, mixed_tile_total_bytes(counts), float(cols[j, 0]),
                                        float(cols[j, 1]), float(cols[j, 2]), float(cols[j, k]), pure, sums=sums[0][j, :6].copy()))
        st["x"] = None
        return results

    def run(self, x3d, numel: int | None = None, maps=None) -> list[TensorResult]:
        """One batch (count, rows, cols): enqueue, finish."""
        return self.finish(self.enqueue(x3d, numel, maps=maps))

    def run_batches(self, batches) -> list[list[TensorResult]]:
        """Batches of any shapes, as `(x3d, numel | None)` pairs or bare tensors: every batch's launches are enqueued first (each with
        its own buffers), then the results are fetched batch by batch.  Same results as run() per batch; `maps_dev` is the last
        batch's."""
        items = [(b, None) if not isinstance(b, (tuple, list)) else (b[0], b[1]) for b in batches]
        states = [self.enqueue(x, n, slot=slot) for slot, (x, n) in enumerate(items)]
        return [self.finish(st) for st in states]
