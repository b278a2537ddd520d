"""`transpose`: every requested format applied to np.transpose(x) and transposed back — does the shared exponent do better along the
weight's other axis? (reference compression_algorithms/transpose.py:13-33).

The mxfp4 / nvfp4 proxies are elementwise, so their transpose rows are their `none` rows bit for bit (the columns from one fp4_proxy_sums
pass, y from mtq_quantize).  np.transpose reverses all axes and quantize_dequantize_bfp_ttnn shares one exponent per 16 elements of the LAST
axis, so with
d0 = x.shape[0] (1 for a 0-d tensor) and V = x.reshape(d0, -1):

    transpose_y(x) == quantize(V.T).T.reshape(x.shape)

— a group is 16 consecutive rows of one column of V, for every rank (1-d and 0-d tensors give the `none` result).  On the hip backend
V is a view of the device tensor: y comes from K2T (mtq_quantize_transposed) and the pcc / mae / atol columns of every mixed-tile
format from ONE K1T pass (mtq_tile_stats_transposed) over all of them, summed as the `none` rows are; no transposed copy is made.
params["materialize_y"] = False skips K2T (y = None, the columns stay).  Reconstructions are cached as `none` caches them.
"""
from __future__ import annotations

import numpy as np

from .base import CompressionAlgorithm, CompressionResult
from .none import _to_host
from .tile_utils import MIXED_TILE_FORMATS


def _columns_hip(v2d, formats: list) -> dict:
    """fmt → {pcc, mae, atol} of the transposed reconstruction of the device matrix v2d, from one K1T pass (float64 moments)."""
    from .. import hip_backend as hb
    from ..pipeline_common import gated_pcc
    from .tile_search import fp0_columns, fmt_mask

    out = {}
    mixed = [f for f in formats if f in MIXED_TILE_FORMATS]
    if mixed:
        mask = fmt_mask(mixed)
        stats = hb.tile_stats_transposed(v2d, mask)
        host = None
        for f in mixed:
            amap = np.full(stats.shape[0], MIXED_TILE_FORMATS.index(f), dtype=np.int8)
            try:
                c = hb.columns_from_stats_device(stats, mask, amap, float(v2d.numel()))
            except hb.MtqError:
                # the device route reads Σx = NaN beside a finite Σx² as a map naming a missing format; with +Inf and −Inf in x
                # that is the true sum: the same records are summed on the host instead
                host = stats.cpu().numpy() if host is None else host
                c = hb.columns_from_stats(host, mask, amap, float(v2d.numel()))
            pcc = gated_pcc(c["pcc"], c["sums"], v2d.numel(), v2d, lambda: hb.quantize_transposed(v2d, f))
            out[f] = {"pcc": pcc, "mae": c["mae"], "atol": c["atol"]}
    if "fp0" in formats:
        pcc, mae, atol = fp0_columns(v2d)
        out["fp0"] = {"pcc": pcc, "mae": mae, "atol": atol}
    proxies = [f for f in formats if f in hb.PROXY_FORMATS]
    if proxies:
        for f, (pcc, mae, atol) in hb.fp4_proxy_columns(v2d, proxies)[0].items():
            out[f] = {"pcc": pcc, "mae": mae, "atol": atol}
    return out


class TransposeCompression(CompressionAlgorithm):
    name = "transpose"

    def _run_emulation(self, xf, formats: list, quantizer, cache) -> list:
        results = []
        xf_t = np.transpose(np.asarray(xf, dtype=np.float32))
        for fmt in formats:
            y = cache.load_array(self.name, fmt)
            if y is not None and y.shape != np.shape(xf):
                y = None
            if y is None:
                y = np.transpose(quantizer.quantize(xf_t, fmt))
                cache.save_array(self.name, fmt, y)
            results.append(CompressionResult(fmt=fmt.upper(), compression=self.name, y=y))
        return results

    def _run_hip(self, xf, formats: list, cache) -> list:
        import torch

        from .. import hip_backend as hb

        was_np = not isinstance(xf, torch.Tensor)
        if was_np:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(xf, dtype=np.float32))).cuda()
        else:
            x = xf if xf.dtype in (torch.bfloat16, torch.float32) else xf.float()
            if not x.is_cuda:
                x = x.cuda()
        shape = tuple(x.shape)
        if x.numel() == 0:   # nothing to quantise: y is the empty tensor, the columns are those of an empty reconstruction
            y = np.zeros(shape, dtype=np.float32) if was_np else torch.zeros(shape, dtype=torch.float32, device=x.device)
            return [CompressionResult(fmt=f.upper(), compression=self.name, y=y) for f in formats]
        d0 = shape[0] if len(shape) else 1
        v = x.reshape(d0, x.numel() // d0)
        if v.stride(-1) != 1:
            v = v.contiguous()
        cols = _columns_hip(v, formats)
        materialize = bool(self.params.get("materialize_y", True))
        results = []
        for fmt in formats:
            y = None
            if materialize:
                cached = cache.load_array(self.name, fmt)
                if cached is not None and cached.shape == shape:
                    y = cached if was_np else torch.from_numpy(cached).to(x.device)
                else:
                    y = (hb.quantize(v, fmt) if fmt in hb.PROXY_FORMATS else hb.quantize_transposed(v, fmt)).reshape(shape)
                    host = _to_host(y)
                    cache.save_array(self.name, fmt, host)
                    if was_np:
                        y = host
            results.append(CompressionResult(fmt=fmt.upper(), compression=self.name, y=y, meta={"columns": cols[fmt]}))
        return results

    def run(self, xf, formats: list, quantizer, cache) -> list:
        if quantizer.backend == "hip":
            return self._run_hip(xf, formats, cache)
        return self._run_emulation(xf, formats, quantizer, cache)
