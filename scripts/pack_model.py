#!/usr/bin/env python3
"""Search a model's tile maps under a compression config and write the packed weights the maps promise.

  pack_model.py MODEL [FILTER ...] --compression-config CFG --out-dir DIR [--backend hip|emulation] [--verify] [--limit N]

MODEL and FILTER are wq's: 'synthetic:<preset>[:seed]' or a local directory of *.safetensors, and an optional name filter.  DIR gets one
<slug>.npz per tensor (packed.save) and an index.json (packed.save_dir) that also records the run (algorithm, parameters, the seed used)
and, per tensor, the size model's bytes and the search's metric value; packed.load_dir reads it back.

--backend hip with mixed-tile-greedy or mixed-tile-threshold: the 2-D tensors are grouped by (shape, storage) as the streamed wq does, a
group's resident batch goes through the search pipeline, and the same batch and the results' maps go to packed.pack_batch: the offsets on
the device, one pack launch, one arena per batch.  Every other tensor or algorithm (vectors, mixed-tile-random, the emulation backend)
takes the per-tensor path: the algorithm's run() and packed.pack.

--verify unpacks what was packed and compares it bit for bit with the reconstruction: K3 (apply_assignment) on the batched path, the
algorithm's own y on the per-tensor path.  A mismatch is reported per tensor and the exit status is 2.

The packed format is the row layout: a config with "layout": "transpose" is refused (exit status 1)."""
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

MIXED_ALGOS = ("mixed-tile-greedy", "mixed-tile-threshold", "mixed-tile-random")


def _bits(y) -> np.ndarray:
    y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
    return np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)


def _differing(got, want) -> int:
    """Words of `got` that are not `want`'s; -1 for another shape."""
    g, w = _bits(got), _bits(want)
    return int(np.count_nonzero(g != w)) if g.shape == w.shape else -1


class _Packer:
    """The run: tensors in, {name: PackedTensor} and their index entries out."""

    def __init__(self, index, algo, formats, backend: str, verify: bool, cache_root: Path):
        self.index, self.algo, self.formats, self.backend, self.verify = index, algo, formats, backend, verify
        self.quantizer = Quantizer(backend=backend)
        self.cache_root = cache_root
        self.named, self.meta, self.mismatches = {}, {}, []
        self.batches = 0

    def _add(self, name: str, pt, metric_value, route: str, differing) -> None:
        counts = pt.counts()
        model = float(mixed_tile_total_bytes(counts))
        self.named[name] = pt
        self.meta[name] = {"size_model_bytes": model, "metric": self.algo.params.get("metric", "pcc"),
                           "metric_value": None if metric_value is None else float(metric_value), "route": route}
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
        pt = packed.pack(x, meta["assignment"], backend=self.backend)
        value = meta.get("metric_value", (meta.get("columns") or {}).get(self.algo.params.get("metric", "pcc")))
        differing = _differing(packed.unpack(pt, backend=self.backend), res.y) if self.verify else None
        self._add(name, pt, value, "per-tensor", differing)

    def batched(self, names: list) -> None:
        """The streamed route's groups: the search pipeline over a resident batch, then pack_batch on the same batch and the results' maps."""
        import torch

        from quantization_analysis_amd import hip_backend as hb
        from quantization_analysis_amd.pipeline import GreedyPipeline, ThresholdPipeline, default_workers

        device = torch.device("cuda", torch.cuda.current_device())
        a = self.algo
        tile_formats = a.tile_formats or [f for f in self.formats if f in MIXED_TILE_FORMATS]
        groups: dict = {}
        for name in names:
            groups.setdefault(streamed.group_key(self.index, name), []).append(name)
        if a.name == "mixed-tile-greedy":
            pipe = GreedyPipeline(tile_formats, a.metric, a.threshold, a.seed, chunk=1, workers=default_workers())
        else:
            pipe = ThresholdPipeline(tile_formats, a.metric, a.threshold, chunk=1)
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
                    maps = np.stack([r.assignment for r in results])
                    pts = packed.pack_batch(x3d, maps, backend="hip", shapes=[tuple(x.shape) for x in xs])
                    self.batches += 1
                    y = packed.unpack_batch(pts, backend="hip") if self.verify else None
                    for i, (name, r, pt) in enumerate(zip(part, results, pts)):
                        differing = _differing(y[i], hb.apply_assignment(x3d[i], r.assignment)) if self.verify else None
                        self._add(name, pt, r.metric_value, "batched", differing)
                    del xs, x3d, y


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
    args = p.parse_args(argv)

    try:
        config = load_compression_config(args.compression_config)
        params = dict(config.params)
        used_seed, seed_source = resolve_seed(config, params)
        algo = create_algorithm(config.algorithm, params)
        if algo.name not in MIXED_ALGOS:
            raise MtqError(f"algorithm {algo.name!r} writes no tile map: pack_model needs one of {', '.join(MIXED_ALGOS)}")
        packed.check_layout(getattr(algo, "layout", "rows"))
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
    run = _Packer(index, algo, formats, args.backend, args.verify, out_dir / "cache")
    print(f"{index.repo_id} @{index.revision} - {len(names)} tensors, {algo.name} {params}, backend {args.backend}")
    try:
        batch_names = []
        if streamed.streamable(algo, formats, args):
            if args.backend == "hip":
                from quantization_analysis_amd import hip_backend as hb

                hb.require_gpu()
            batch_names = [n for n in names if streamed.group_key(index, n) is not None]
            run.batched(batch_names)
        for name in names:
            if name not in run.named:
                run.per_tensor(name)
    except MtqError as exc:
        print(f"error: {exc}")
        return 1
    named = {n: run.named[n] for n in names}
    info = {"model": index.repo_id, "revision": index.revision, "algorithm": algo.name, "params": params, "seed": used_seed, "seed_source": seed_source,
            "backend": args.backend, "formats": list(formats)}
    packed.save_dir(out_dir, named, meta=run.meta, run=info)
    total = sum(pt.nbytes for pt in named.values())
    total_all = sum(pt.total_bytes for pt in named.values())
    model = sum(m["size_model_bytes"] for m in run.meta.values())
    bf16 = sum(2.0 * 1024 * pt.map.size for pt in named.values())
    print(f"wrote {out_dir}: {len(named)} tensors ({len(batch_names)} in {run.batches} batches, {len(named) - len(batch_names)} one by one)")
    print(f"total packed bytes {total} (+ {total_all - total} of maps and offsets) ratio to bf16 {total / bf16:.5f}; "
          f"size-model bytes {model:.1f} ratio to bf16 {model / bf16:.5f}")
    if run.mismatches:
        print(f"verify: MISMATCH in {len(run.mismatches)} tensors: {', '.join(run.mismatches)}")
        return 2
    if args.verify:
        print(f"verify: ok ({len(named)} tensors equal the reconstruction bit for bit)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
