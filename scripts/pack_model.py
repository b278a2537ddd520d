#!/usr/bin/env python3
"""Search a model's tile maps under a compression config and write the packed weights the maps promise.

  pack_model.py MODEL [FILTER ...] --compression-config CFG --out-dir DIR [--backend hip|emulation] [--verify] [--limit N]
                [--store-transposed]

MODEL and FILTER are wq's: 'synthetic:<preset>[:seed]' or a local directory of *.safetensors, and an optional name filter.  DIR gets one
<slug>.npz per tensor (packed.save) and an index.json (packed.save_dir) that also records the run (algorithm, parameters, the seed used)
and, per tensor, the size model's bytes and the search's metric value; packed.load_dir reads it back.

--backend hip with mixed-tile-greedy or mixed-tile-threshold: the 2-D tensors are grouped by (shape, storage) as the streamed wq does, a
group's resident batch goes through the search pipeline, and the same batch and the results' maps go to packed.pack_batch: the offsets on
the device, one pack launch, one arena per batch.  Every other tensor or algorithm (vectors, mixed-tile-random, the emulation backend)
takes the per-tensor path: the algorithm's run() and packed.pack.

--verify unpacks what was packed and compares it bit for bit with the reconstruction: K3 (apply_assignment) on the batched path, the
algorithm's own y on the per-tensor path.  A mismatch is reported per tensor and the exit status is 2.

The packed format is the row layout: a config with "layout": "transpose" is refused (exit status 1) unless --store-transposed is given.

--store-transposed (only with a "layout": "transpose" config; exit status 1 otherwise): every tensor's TRANSPOSE is packed under the map
the search wrote for it, as pack_mixed_tile_assignment.py --store-transposed does for one tensor.  On hip with greedy or threshold the
2-D tensors are grouped as above, the resident batch goes through the pipeline built with layout="transpose" and, with the results'
maps, to packed.pack_batch_transposed, which reads it in place; --verify compares packed.unpack_batch_transposed with K3T
(apply_assignment_transposed).  Every other case takes the per-tensor path: the algorithm's run() with the layout in its params, then
packed.pack_transposed (2-D) or packed.pack of the permuted copy np.transpose(x) (other ranks; a vector is its own transpose), verified
against the algorithm's own y brought to the stored orientation.

mixed-tile-budget (params: bits, scope): with "scope": "tensor" every tensor gets its own budget of bits / 8 bytes per weight of its
tiles and the routes are those above (on hip the 2-D tensors go through pipeline.BudgetPipeline and its device maps straight to
packed.pack_batch).  With "scope": "model" ONE budget of bits / 8 · 1024 · (all tiles) bytes covers the whole selection, tiles numbered
through in the order of the names, so a sensitive tensor takes bytes from an insensitive one: on hip the shape groups are streamed once for
their weight-space error tables (32 B per tile stay on the device), one mtq_budget_allocate_device call with one segment allocates, and
the groups are streamed again for the columns, pack_batch and --verify; on emulation budget_maps.model_maps does the same on the host.
index.json records bits, scope, the budget and the achieved size-model bytes, and the summary prints the achieved bits per weight.

Every --store-transposed index entry says "stored": "transpose" and keeps the tensor's
own shape as "source_shape"; "shape" is the packed tensor's, so packed.load_dir reads the directory as any other and its 2-D entries,
of shape (k, n), go to packed.PackedMatmul (packed.read_index shows which entries those are)."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np

from quantization_analysis_amd import packed, streamed
from quantization_analysis_amd.cli import resolve_seed
from quantization_analysis_amd.compression_algorithms import create_algorithm, load_compression_config
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS, mixed_tile_total_bytes
from quantization_analysis_amd.hip_backend import MtqError
from quantization_analysis_amd.model_source import build_model_index, resolve_format_list, resolve_selected_tensors
from quantization_analysis_amd.quantization_formats import SUPPORTED_FORMATS

MIXED_ALGOS = ("mixed-tile-greedy", "mixed-tile-threshold", "mixed-tile-random", "mixed-tile-budget")


def _host(y) -> np.ndarray:
    y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
    return np.ascontiguousarray(y, dtype=np.float32)


def _bits(y) -> np.ndarray:
    return _host(y).view(np.uint32)


def _differing(got, want) -> int:
    """Words of `got` that are not `want`'s; -1 for another shape."""
    g, w = _bits(got), _bits(want)
    return int(np.count_nonzero(g != w)) if g.shape == w.shape else -1


class _Packer:
    """The run: tensors in, {name: PackedTensor} and their index entries out."""

    def __init__(self, index, algo, formats, backend: str, verify: bool, cache_root: Path, transposed: bool = False):
        self.index, self.algo, self.formats, self.backend, self.verify = index, algo, formats, backend, verify
        self.transposed = transposed                 # --store-transposed: the packed tensors are the transposes'
        self.quantizer = Quantizer(backend=backend)
        self.cache_root = cache_root
        self.named, self.meta, self.mismatches = {}, {}, []
        self.batches = 0

    def _add(self, name: str, pt, metric_value, route: str, differing, source_shape=None) -> None:
        counts = pt.counts()
        model = float(mixed_tile_total_bytes(counts))
        self.named[name] = pt
        self.meta[name] = {"size_model_bytes": model, "metric": self.algo.params.get("metric", "pcc"),
                           "metric_value": None if metric_value is None else float(metric_value), "route": route}
        if self.transposed:
            self.meta[name].update(stored="transpose", source_shape=[int(v) for v in source_shape])
        if differing is not None:
            self.meta[name]["verified"] = differing == 0
            if differing != 0:
                self.mismatches.append(name)
        state = "" if differing is None else ("  verify: ok" if differing == 0 else f"  verify: MISMATCH ({differing} words differ from the reconstruction)")
        print(f"{name} {pt.shape} {route}: packed bytes {pt.nbytes} (+ {pt.total_bytes - pt.nbytes} of map and offsets), size-model bytes {model:.1f}{state}")

    def per_tensor(self, name: str) -> None:
        """The algorithm's run() on one tensor, then packed.pack."""
        if self.backend == "hip":
            import torch

            x = self.index.load(name, device=torch.device("cuda", torch.cuda.current_device()))
        else:
            x = np.asarray(self.index.load(name).float().numpy(), dtype=np.float32)
        cache = CacheContext(root=self.cache_root, tensor_name=name, backend=self.backend, recompute=True, run_tag="pack")
        res = next(r for r in self.algo.run(xf=x, formats=self.formats, quantizer=self.quantizer, cache=cache) if r.fmt == "MIXED")
        meta = res.meta or {}
        want = res.y
        if not self.transposed:
            pt = packed.pack(x, meta["assignment"], backend=self.backend)
        else:                                        # the stored orientation is np.transpose(x)'s, the one the map was written over
            if len(x.shape) == 2:
                pt = packed.pack_transposed(x, meta["assignment"], backend=self.backend)
            else:
                xt = x.permute(*reversed(range(x.dim()))).contiguous() if self.backend == "hip" else np.ascontiguousarray(np.transpose(x))
                pt = packed.pack(xt, meta["assignment"], backend=self.backend)
            want = np.transpose(_host(want)) if self.verify else None
        value = meta.get("metric_value", (meta.get("columns") or {}).get(self.algo.params.get("metric", "pcc")))
        differing = _differing(packed.unpack(pt, backend=self.backend), want) if self.verify else None
        self._add(name, pt, value, "per-tensor", differing, source_shape=tuple(x.shape))

    def batched(self, names: list) -> None:
        """The streamed route's groups: the search pipeline over a resident batch, then pack_batch (--store-transposed: the transposed
        pipeline and pack_batch_transposed) on the same batch and the results' maps."""
        import torch

        from quantization_analysis_amd import hip_backend as hb
        from quantization_analysis_amd.pipeline import BudgetPipeline, GreedyPipeline, ThresholdPipeline, default_workers

        device = torch.device("cuda", torch.cuda.current_device())
        a = self.algo
        tile_formats = a.tile_formats or [f for f in self.formats if f in MIXED_TILE_FORMATS]
        groups: dict = {}
        for name in names:
            groups.setdefault(streamed.group_key(self.index, name, layout=a.layout), []).append(name)
        if a.name == "mixed-tile-greedy":
            pipe = GreedyPipeline(tile_formats, a.metric, a.threshold, a.seed, chunk=1, workers=default_workers(), layout=a.layout)
        elif a.name == "mixed-tile-budget":
            pipe = BudgetPipeline(tile_formats, a.metric, a.bits, chunk=1)
        else:
            pipe = ThresholdPipeline(tile_formats, a.metric, a.threshold, chunk=1, layout=a.layout)
        with pipe:
            for (rows, cols, _dtype), items in groups.items():
                tiles = -(-rows // 32) * -(-cols // 32)
                per_batch = max(1, streamed.MAX_BATCH_TILES // tiles)
                for b0 in range(0, len(items), per_batch):
                    part = items[b0:b0 + per_batch]
                    xs = [self.index.load(n, device=device) for n in part]
                    x3d = torch.stack([x.reshape(rows, cols) for x in xs])
                    pipe.chunk = min(max(1, streamed.K1_LAUNCH_TILES // tiles), len(part))
                    results = pipe.run(x3d)
                    if a.name == "mixed-tile-budget":         # the allocator's maps never left the device
                        maps = pipe.maps_dev.view(len(part), *results[0].assignment.shape)
                    else:
                        maps = np.stack([r.assignment for r in results])
                    if self.transposed:
                        pts = packed.pack_batch_transposed(x3d, maps, backend="hip")
                        unpack_batch, k3 = packed.unpack_batch_transposed, hb.apply_assignment_transposed
                    else:
                        pts = packed.pack_batch(x3d, maps, backend="hip", shapes=[tuple(x.shape) for x in xs])
                        unpack_batch, k3 = packed.unpack_batch, hb.apply_assignment
                    self.batches += 1
                    y = unpack_batch(pts, backend="hip") if self.verify else None
                    for i, (name, r, pt) in enumerate(zip(part, results, pts)):
                        differing = _differing(y[i], k3(x3d[i], r.assignment)) if self.verify else None
                        self._add(name, pt, r.metric_value, "batched", differing, source_shape=tuple(xs[i].shape))
                    del xs, x3d, y

    # ------------------------------------------------------------------------- mixed-tile-budget, scope "model"

    def _grid(self, name: str) -> tuple:
        """The tile grid of a tensor's 2-D flatten (tile_utils.flatten_2d), from its shape alone."""
        shape, _dtype = self.index.shape_dtype(name)
        rows, cols = (1, 1) if len(shape) == 0 else ((-(-int(shape[0]) // 32), 32) if len(shape) == 1 else (int(np.prod(shape[:-1])), int(shape[-1])))
        return -(-rows // 32), -(-cols // 32)

    def model_scope(self, names: list) -> dict:
        """One budget over all of `names` → what index.json records of it (budget_bytes, tiles).  Raises MtqError with allocate's reason
        when no map is made."""
        from quantization_analysis_amd import budget_maps as bm
        from quantization_analysis_amd.compression_algorithms import mixed_tile_budget as mtb
        from quantization_analysis_amd.compression_algorithms.tile_search import columns_from_stats, compute_tile_stats, reconstruct

        a = self.algo
        tile_formats = a.candidates(self.formats)
        grids = [self._grid(n) for n in names]
        first = np.concatenate([[0], np.cumsum([th * tw for th, tw in grids])]).astype(np.int64)
        total = int(first[-1])
        where = {n: j for j, n in enumerate(names)}
        budget = bm.model_budget(a.bits, total)
        metric = a.metric
        if self.backend != "hip":
            xs = {n: np.asarray(self.index.load(n).float().numpy(), dtype=np.float32) for n in names}
            stats = {n: compute_tile_stats(xs[n], tile_formats, self.quantizer) for n in names}
            tables = [bm.tile_error_tables_emulation(stats[n].x2d, np.zeros((grids[where[n]][1], 32, 32)))[1] for n in names]
            got = bm.model_maps(tables, grids, tile_formats, a.bits)
            if isinstance(got, str):
                raise MtqError(got)
            for n, amap in zip(names, got[0]):
                pt = packed.pack(xs[n], amap, backend=self.backend)
                differing = _differing(packed.unpack(pt, backend=self.backend), reconstruct(stats[n], amap, self.quantizer)) if self.verify else None
                self._add(n, pt, columns_from_stats(stats[n], amap)[metric], "model-scope", differing)
            return {"budget_bytes": budget, "tiles": total}

        import torch

        from quantization_analysis_amd import hip_backend as hb
        from quantization_analysis_amd.pipeline import BudgetPipeline

        device = torch.device("cuda", torch.cuda.current_device())
        batches = []                                             # (names of one resident batch, (rows, cols) or None for a tensor alone)
        groups: dict = {}
        for n in names:
            groups.setdefault(streamed.group_key(self.index, n), []).append(n)
        for key, items in groups.items():
            if key is None:
                batches += [([n], None) for n in items]
                continue
            per_batch = max(1, streamed.MAX_BATCH_TILES // (-(-key[0] // 32) * -(-key[1] // 32)))
            batches += [(items[b0:b0 + per_batch], (key[0], key[1])) for b0 in range(0, len(items), per_batch)]

        def resident(part, hw):
            """→ (the tensors as loaded, their (count, rows, cols) batch, element count of one, shape infos)."""
            xs = [self.index.load(n, device=device) for n in part]
            if hw is not None:
                return xs, torch.stack([x.reshape(*hw) for x in xs]), None, None
            x2d, info = hb.to_device_2d(xs[0])
            return xs, x2d[None], int(xs[0].numel()), info

        # phase 1: every tile's four errors, on the device
        table = torch.empty((total, 4), dtype=torch.float64, device=device)
        for part, hw in batches:
            _xs, x3d, _numel, _info = resident(part, hw)
            t = hb.tile_sq_error_batched(x3d)
            for i, n in enumerate(part):
                table[int(first[where[n]]):int(first[where[n] + 1])] = t[i]
            del _xs, x3d, t
        # phase 2: one segment over everything
        maps, counts, status = hb.budget_allocate_device(table, torch.tensor([0, total], dtype=torch.int64, device=device), tile_formats,
                                                         torch.tensor([budget], dtype=torch.float64, device=device))
        reason = mtb.status_reason(int(status.cpu()[0]), tile_formats, a.bits, total)
        if reason is not None:
            raise MtqError(reason)
        self.model_table, self.model_map = table, maps          # kept for callers that check the allocation (tests)
        # phase 3: the columns, the packed streams and the check, group by group under the allocated maps
        with BudgetPipeline(tile_formats, metric, a.bits, chunk=1) as pipe:
            for part, hw in batches:
                xs, x3d, numel, info = resident(part, hw)
                bmaps = torch.stack([maps[int(first[where[n]]):int(first[where[n] + 1])] for n in part])
                results = pipe.run(x3d, numel=numel, maps=bmaps)
                self.batches += 1
                if hw is not None:
                    pts = packed.pack_batch(x3d, bmaps.view(len(part), *grids[where[part[0]]]), backend="hip", shapes=[tuple(x.shape) for x in xs])
                    y = packed.unpack_batch(pts, backend="hip") if self.verify else None
                    for i, (n, r, pt) in enumerate(zip(part, results, pts)):
                        differing = _differing(y[i], hb.apply_assignment(x3d[i], r.assignment)) if self.verify else None
                        self._add(n, pt, r.metric_value, "model-scope batched", differing)
                else:
                    r = results[0]
                    pt = packed.pack(xs[0], r.assignment, backend="hip")
                    want = hb.unflatten(hb.apply_assignment(x3d[0], r.assignment), info) if self.verify else None
                    differing = _differing(packed.unpack(pt, backend="hip"), want) if self.verify else None
                    self._add(part[0], pt, r.metric_value, "model-scope", differing)
                del xs, x3d
        return {"budget_bytes": budget, "tiles": total}


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Search a model's tile maps and write the packed weights.")
    p.add_argument("repo_or_url", help="'synthetic:<preset>[:seed]' or a local directory of *.safetensors.")
    p.add_argument("filter_query", nargs="*", help="Optional filter: substring, or dotted torch-style prefix path.")
    p.add_argument("--compression-config", required=True, help="Path to a JSON compression config of a mixed-tile algorithm.")
    p.add_argument("--out-dir", required=True, help="Directory of the packed tensors and their index.json.")
    p.add_argument("--backend", choices=list(packed.BACKENDS), default="emulation")
    p.add_argument("--revision", default="main")
    p.add_argument("--limit", type=int, default=None, help="Optional max matched tensors.")
    p.add_argument("--verify", action="store_true", help="Unpack every tensor and compare it bit for bit with the reconstruction.")
    p.add_argument("--store-transposed", action="store_true",
                   help='With a "layout": "transpose" config: pack every tensor\'s transpose under its map (2-D tensors become (k, n) row-layout tensors).')
    args = p.parse_args(argv)

    try:
        config = load_compression_config(args.compression_config)
        params = dict(config.params)
        used_seed, seed_source = resolve_seed(config, params)
        algo = create_algorithm(config.algorithm, params)
        if algo.name not in MIXED_ALGOS:
            raise MtqError(f"algorithm {algo.name!r} writes no tile map: pack_model needs one of {', '.join(MIXED_ALGOS)}")
        layout = getattr(algo, "layout", "rows")
        if args.store_transposed and layout != "transpose":
            raise MtqError('--store-transposed packs the tensors\' transposes under maps written for "layout": "transpose"; this config\'s '
                           f"layout is {layout!r}")
        if not args.store_transposed:
            packed.check_layout(layout)
        formats = resolve_format_list(config.quantization_formats, SUPPORTED_FORMATS)
        index = build_model_index(args.repo_or_url, revision=args.revision)
        try:
            names = resolve_selected_tensors(index, " ".join(args.filter_query).strip() or None)
        except RuntimeError:
            names = []
        if args.limit is not None:
            names = names[: max(0, args.limit)]
        if not names:
            raise MtqError("No tensors matched.")
    except (MtqError, ValueError, FileNotFoundError) as exc:
        print(f"error: {exc}")
        return 1

    out_dir = Path(args.out_dir)
    run = _Packer(index, algo, formats, args.backend, args.verify, out_dir / "cache", transposed=args.store_transposed)
    print(f"{index.repo_id} @{index.revision} - {len(names)} tensors, {algo.name} {params}, backend {args.backend}")
    try:
        batch_names = []
        budget_info = None
        if algo.name == "mixed-tile-budget" and algo.scope == "model":
            if args.backend == "hip":
                from quantization_analysis_amd import hip_backend as hb

                hb.require_gpu()
            budget_info = run.model_scope(names)
        elif streamed.streamable(algo, formats, args):
            if args.backend == "hip":
                from quantization_analysis_amd import hip_backend as hb

                hb.require_gpu()
            batch_names = [n for n in names if streamed.group_key(index, n, layout=layout) is not None]
            run.batched(batch_names)
        for name in names:
            if name not in run.named:
                run.per_tensor(name)
    except (MtqError, ValueError) as exc:
        print(f"error: {exc}")
        return 1
    named = {n: run.named[n] for n in names}
    info = {"model": index.repo_id, "revision": index.revision, "algorithm": algo.name, "params": params, "seed": used_seed, "seed_source": seed_source,
            "backend": args.backend, "formats": list(formats), **({"layout": layout, "stored": "transpose"} if args.store_transposed else {})}
    model = sum(m["size_model_bytes"] for m in run.meta.values())
    if algo.name == "mixed-tile-budget":
        tiles = sum(pt.map.size for pt in named.values())
        if budget_info is None:                               # scope "tensor": the budgets of the tensors, each kept on its own
            from quantization_analysis_amd import budget_maps as bm

            budget_info = {"budget_bytes": float(sum(bm.model_budget(algo.bits, pt.map.size) for pt in named.values())), "tiles": tiles}
        totals = {f: sum(pt.counts()[f] for pt in named.values()) for f in MIXED_TILE_FORMATS}
        model = float(mixed_tile_total_bytes(totals))         # the size model of all tiles at once, as the model scope's allocation sums it
        info.update(bits=algo.bits, scope=algo.scope, budget_bytes=budget_info["budget_bytes"], size_model_bytes=model,
                    achieved_bits=model * 8.0 / (1024.0 * tiles))
    packed.save_dir(out_dir, named, meta=run.meta, run=info)
    total = sum(pt.nbytes for pt in named.values())
    total_all = sum(pt.total_bytes for pt in named.values())
    bf16 = sum(2.0 * 1024 * pt.map.size for pt in named.values())
    print(f"wrote {out_dir}: {len(named)} tensors ({len(batch_names)} in {run.batches} batches, {len(named) - len(batch_names)} one by one)")
    print(f"total packed bytes {total} (+ {total_all - total} of maps and offsets) ratio to bf16 {total / bf16:.5f}; "
          f"size-model bytes {model:.1f} ratio to bf16 {model / bf16:.5f}")
    if algo.name == "mixed-tile-budget":
        print(f"budget: {algo.bits:g} bits per weight, scope {algo.scope}: {info['budget_bytes']:.1f} B; achieved {info['achieved_bits']:.5f} bits per weight "
              f"({model:.1f} size-model bytes)")
    if run.mismatches:
        print(f"verify: MISMATCH in {len(run.mismatches)} tensors: {', '.join(run.mismatches)}")
        return 2
    if args.verify:
        print(f"verify: ok ({len(named)} tensors equal the reconstruction bit for bit)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
