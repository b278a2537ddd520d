"""Layer-output error of quantised weights on recorded activations.

For one op with weight W (n × k, nn.Linear convention) and activations X (m × k, bf16) the reference output is R = X·Wᵀ (+ b) and
every candidate f gives Y_f = X·Ŵ_fᵀ (+ b): Ŵ_f = quantize_weight_values(W, f) in the row layout for a pure format, the search's
reconstruction for the map of a mixed-tile algorithm, Y = b (or 0) for fp0.  Each row reports pcc, mae and atol of Y_f against R
over all m·n outputs, from the seven float64 sums mtq_columns_from_sums takes (so its zero-denominator rule is the one of the
searches); the `recorded` row compares R with the op's recorded output.  atol follows np.max: a NaN anywhere in |r − q| (a NaN
recorded output, an Inf weight giving ∞ − ∞) makes that row's atol NaN on both backends, whichever M-chunk holds it.

Activation formats (x_format): with bfp8 / bfp4 / bfp2 every candidate but fp0 is fed Q(X) = quantize_weight_values(X, x_format) of
each M-chunk (the row layout: groups of 16 consecutive K elements of one token, so Q(X) does not depend on the chunking) while R keeps
the raw X: Y_f = Q(X)·Ŵ_fᵀ (+ b), the bf16 row Q(X)·bf16(W)ᵀ (+ b).  x_format = "bf16" (the default) is X as recorded.

Transposed layout (transpose=True, a config with the transpose algorithm, or a mixed-tile config with "layout": "transpose"): the
candidates <f>+transpose for each of bfp8 / bfp4 / bfp2 among the formats have Ŵ = quantize_weight_values(Wᵀ, f)ᵀ — a group is 16
consecutive rows (N) of one column (k), aligned from row 0, a ragged last group completed with +0 — which is the transpose algorithm's y.
bf16 and fp0 are elementwise and get no transposed row; the bytes are the row-layout format's.  A map in this layout is over Wᵀ's tile
grid, tiles_hw(k, n): the map of a "layout": "transpose" search (map:<algorithm>+transpose) and the budget maps budget:<B>:<basis>+transpose.
Q(X) keeps X's row layout; only W's layout changes.  GPTQ is row-layout only: its transposed counterparts are listed in budget_skipped.
Row order: the row-layout formats, the +transpose formats, the map, recorded, then per budget the two row-layout maps and their two
transposed maps, then GPTQ.

Backends:
  * hip       — csrc/mtq_output_error.hip: one pass per M-chunk with every candidate's W image built on the fly in LDS, the sums
                reduced in the epilogue; neither Ŵ nor Y is materialised.  A BFP x_format adds one row pre-pass per chunk that writes
                Q(X) as bf16, and the pass takes it as the candidates' A operand.  Transposed candidates add one transposed launch
                (mtq_output_error_transposed) per chunk with only their slots;
  * emulation — the same contract on the host in float64 (torch), from quantization_formats.quantize_weight_values: the oracle of
                the GPU tests and the route for small CPU runs.
"""
from __future__ import annotations

import tempfile
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterable, Optional

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from .layer_io import Chunk, OpIO, check_op, chunks
from .quantization_formats import BASE_FORMATS as SUPPORTED_FORMATS, quantize_weight_values  # no proxy rows here

FORMAT_BYTES_PER_ELEM = {"bf16": 2.0, "bfp8": 1.088, "bfp4": 0.50097, "bfp2": 0.25097, "fp0": 0.0}  # wq:132-140 (cli.py)
SLOTS = ("bf16", "bfp8", "bfp4", "bfp2", "map", "fp0", "recorded")  # include/mtq.h MTQ_OE_*
BACKENDS = ("emulation", "hip")
MIXED_ALGOS = {"mixed-tile-greedy", "mixed-tile-random", "mixed-tile-threshold", "mixed-tile-budget"}
LAYOUTS = ("rows", "transpose")
TRANSPOSE_FORMATS = ("bfp8", "bfp4", "bfp2")   # the formats with a +transpose row: bf16 and fp0 are elementwise
TRANSPOSE_SUFFIX = "+transpose"
X_FORMATS = ("bf16", "bfp8", "bfp4", "bfp2")   # activation formats; bf16 = X as recorded


@dataclass
class MapCandidate:
    """The map of a mixed-tile search over W: `assignment` int8 (tiles_h, tiles_w) of codes into MIXED_TILE_FORMATS, `y` the search's
    reconstruction (host ndarray or device tensor), `tile_bytes` its weight bytes.  layout "transpose": the assignment is over Wᵀ's grid,
    tiles_hw(k, n), and y is in W's orientation."""

    name: str
    assignment: np.ndarray
    y: object
    tile_bytes: float
    layout: str = "rows"


@dataclass
class Row:
    candidate: str
    bytes: Optional[float]
    pcc: float
    mae: float
    atol: float
    sums: tuple = ()
    extra: dict = field(default_factory=dict)   # budget maps: bits, basis, calib_tokens, predicted_sse_calib


@dataclass
class OpResult:
    op: str
    weight: str
    shape: tuple = ()
    m: int = 0
    splits: list = field(default_factory=list)
    x_cast: bool = False
    rows: list = field(default_factory=list)
    skipped: Optional[str] = None
    x_format: str = "bf16"
    budget_skipped: list = field(default_factory=list)   # (candidate, reason) of budget maps that were not made
    calib_splits: list = field(default_factory=list)


def config_layout(config) -> str:
    """"transpose" for a config with the transpose algorithm or "layout": "transpose", else "rows" (None included)."""
    if config is None:
        return "rows"
    if config.algorithm == "transpose" or str((config.params or {}).get("layout", "rows")) == "transpose":
        return "transpose"
    return "rows"


def check_layout(config, layouts=("rows",)) -> None:
    """Raises for a config whose layout is not among `layouts`.  The default admits the row layout only (the routes that have no
    transposed counterpart, GPTQ's); evaluate_op, search_map and the CLI pass LAYOUTS."""
    if config is None:
        return
    if config_layout(config) not in layouts:
        raise ValueError("layer output error supports only the row layout: compression configs with \"layout\": \"transpose\" "
                         "(or the transpose algorithm) are not supported")


def check_x_format(x_format: str) -> None:
    if x_format not in X_FORMATS:
        raise ValueError(f"Unsupported activation format {x_format!r}. Supported: {', '.join(X_FORMATS)}")


def quantize_x(x, x_format: str):
    """Q(X) of one (m, k) chunk on the host as a float64 torch tensor: quantize_weight_values of its float32 values in the row layout."""
    import torch

    check_x_format(x_format)
    x32 = x.float().cpu().numpy()
    return torch.from_numpy(quantize_weight_values(x32, x_format).astype(np.float64))


def search_map(w, config, backend: str, name: str = "weight") -> Optional[MapCandidate]:
    """Runs the config's mixed-tile algorithm on W through the plugin API → its map candidate (None for a config without one)."""
    from .compression_algorithms import create_algorithm
    from .compression_algorithms.cache import CacheContext
    from .compression_algorithms.quantizer import Quantizer
    from .model_source import resolve_format_list

    from .cli import display_name

    if config is None or config.algorithm not in MIXED_ALGOS:
        return None
    check_layout(config, LAYOUTS)
    params = dict(config.params)
    if config.seed is not None:                      # wq's seed rule for a config seed (cli.resolve_seed); params["seed"] otherwise
        params["seed"] = int(config.seed)
    algo = create_algorithm(config.algorithm, params)
    formats = resolve_format_list(config.quantization_formats, SUPPORTED_FORMATS)
    with tempfile.TemporaryDirectory() as tmp:
        cache = CacheContext(root=Path(tmp), tensor_name=name, backend=backend, recompute=True, run_tag="output-error")
        results = algo.run(xf=w, formats=formats, quantizer=Quantizer(backend), cache=cache)
    for res in results:
        if res.fmt == "MIXED" and res.meta and isinstance(res.meta.get("assignment"), np.ndarray) and res.y is not None:
            return MapCandidate(name=f"map:{display_name(algo)}", assignment=np.ascontiguousarray(res.meta["assignment"], dtype=np.int8),
                                y=res.y, tile_bytes=float(res.tile_bytes), layout=config_layout(config))
    raise RuntimeError(f"{config.algorithm} returned no map with a reconstruction")


def _columns(sums7, elem_count: float) -> tuple:
    from .hip_backend import columns_from_sums

    c = columns_from_sums(np.asarray(sums7, dtype=np.float64), elem_count)
    return c["pcc"], c["mae"], c["atol"]


def _fold64(acc: np.ndarray, r, q) -> None:
    """acc[0..6] += Σr, Σr², Σq, Σq², Σrq, Σ|r−q|; acc[6] = max(acc[6], max|r−q|) — float64 torch tensors r, q of one chunk.
    The max propagates NaN whichever chunk holds it (np.max semantics, as the kernel)."""
    d = (r - q).abs()
    acc[0] += float(r.sum())
    acc[1] += float((r * r).sum())
    acc[2] += float(q.sum())
    acc[3] += float((q * q).sum())
    acc[4] += float((r * q).sum())
    acc[5] += float(d.sum())
    if d.numel():
        acc[6] = np.maximum(acc[6], float(d.max()))


def quantize_transposed(w32: np.ndarray, fmt: str) -> np.ndarray:
    """Ŵ of the transposed layout on the host (float32): quantize_weight_values(Wᵀ, f)ᵀ, the transpose algorithm's y of a 2-D W."""
    return np.ascontiguousarray(quantize_weight_values(np.ascontiguousarray(w32.T), fmt).T)


def emulation_sums(chunk_iter: Iterable, w, formats, bias=None, map_y=None, x_format: str = "bf16", t_formats=(),
                   map_t_y=None) -> tuple[np.ndarray, int, bool, bool]:
    """Float64 host route → (sums [7, 7] in SLOTS order, m, any recorded output seen, any cast).  t_formats (⊆ TRANSPOSE_FORMATS) or
    map_t_y (a transposed map's Ŵ) make sums [14, 7]: rows 7.. are the slots of the transposed launch (bfp8 / bfp4 / bfp2 and the map in
    the transposed layout, and fp0)."""
    import torch

    check_x_format(x_format)
    t_formats = [f for f in t_formats if f in TRANSPOSE_FORMATS]
    two = bool(t_formats) or map_t_y is not None

    w32 = np.asarray(w.float().cpu().numpy() if hasattr(w, "cpu") else w, dtype=np.float32)
    w64 = torch.from_numpy(w32.astype(np.float64))
    b64 = None if bias is None else torch.from_numpy(np.asarray(bias.float().cpu().numpy() if hasattr(bias, "cpu") else bias, dtype=np.float64))
    what = {}
    for f in formats:
        if f in MIXED_TILE_FORMATS:
            what[f] = torch.from_numpy(quantize_weight_values(w32, f).astype(np.float64))
    if map_y is not None:
        what["map"] = torch.from_numpy(np.asarray(map_y.float().cpu().numpy() if hasattr(map_y, "cpu") else map_y, dtype=np.float64))
    what_t = {f: torch.from_numpy(quantize_transposed(w32, f).astype(np.float64)) for f in t_formats}
    if map_t_y is not None:
        what_t["map"] = torch.from_numpy(np.asarray(map_t_y.float().cpu().numpy() if hasattr(map_t_y, "cpu") else map_t_y, dtype=np.float64))
    sums = np.zeros((2 * len(SLOTS) if two else len(SLOTS), 7), dtype=np.float64)
    m, seen_rec, cast = 0, False, False
    for ch in chunk_iter:
        x64 = ch.x.to(torch.float64)
        r = x64 @ w64.T
        if b64 is not None:
            r = r + b64
        xq64 = x64 if x_format == "bf16" else quantize_x(ch.x, x_format)
        for slot, wh in what.items():
            q = xq64 @ wh.T
            if b64 is not None:
                q = q + b64
            _fold64(sums[SLOTS.index(slot)], r, q)
        for slot, wh in what_t.items():
            q = xq64 @ wh.T
            if b64 is not None:
                q = q + b64
            _fold64(sums[len(SLOTS) + SLOTS.index(slot)], r, q)
        q0 = torch.zeros_like(r) if b64 is None else b64.expand_as(r)
        _fold64(sums[SLOTS.index("fp0")], r, q0)
        if two:                                      # the transposed launch forms fp0 as well
            _fold64(sums[len(SLOTS) + SLOTS.index("fp0")], r, q0)
        if ch.recorded is not None:
            seen_rec = True
            _fold64(sums[SLOTS.index("recorded")], r, ch.recorded.to(torch.float64))
        m += int(ch.x.shape[0])
        cast = cast or ch.cast
    return sums, m, seen_rec, cast


def hip_sums(chunk_iter: Iterable, w, formats, bias=None, assignment=None, x_format: str = "bf16", t_formats=(),
             t_assignment=None) -> tuple[np.ndarray, int, bool, bool]:
    """The fused kernel over every chunk, partial sums carried on the device → the same as emulation_sums.  A BFP x_format quantises
    each chunk's X into one reused bf16 buffer first.  t_formats / t_assignment (a map over Wᵀ's grid) add one transposed launch per
    chunk with their slots alone, into rows 7.. of sums [14, 7]; the row launch is skipped when it has no slot of its own to fill."""
    import torch

    from . import hip_backend as hb

    check_x_format(x_format)

    dev = torch.device("cuda", torch.cuda.current_device())
    wd = w.to(dev) if w.dtype in (torch.bfloat16, torch.float32) else w.float().to(dev)
    wd = wd if wd.stride(-1) == 1 else wd.contiguous()
    bd = None if bias is None else bias.float().contiguous().to(dev)
    ad = None if assignment is None else torch.from_numpy(np.ascontiguousarray(assignment, dtype=np.int8)).to(dev)
    mask = hb.fmt_mask([f for f in formats if f in MIXED_TILE_FORMATS])
    t_mask = hb.fmt_mask([f for f in t_formats if f in TRANSPOSE_FORMATS]) if t_formats else 0
    tad = None if t_assignment is None else torch.from_numpy(np.ascontiguousarray(t_assignment, dtype=np.int8)).to(dev)
    two = bool(t_mask) or tad is not None
    sums = torch.zeros((2 * len(SLOTS) if two else len(SLOTS), 7), dtype=torch.float64, device=dev)
    scratch = xq_buf = None
    m, seen_rec, cast = 0, False, False
    for ch in chunk_iter:
        xd = ch.x.to(dev, non_blocking=False).contiguous()
        rd = None
        if ch.recorded is not None:
            seen_rec = True
            rd = ch.recorded.to(dev)
            rd = rd if rd.dtype in (torch.bfloat16, torch.float32) else rd.float()
            rd = rd.contiguous()
        need = hb.output_error_scratch(int(xd.shape[0]), int(wd.shape[0]))
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty((need,), dtype=torch.float64, device=dev)
        xq = None
        if x_format != "bf16":
            if xq_buf is None or xq_buf.numel() < xd.numel():
                xq_buf = torch.empty((xd.numel(),), dtype=torch.bfloat16, device=dev)
            xq = hb.quantize_rows_bf16(xd, x_format, out=xq_buf[: xd.numel()].view(xd.shape))
        if not two or mask or ad is not None or rd is not None:
            hb.output_error(xd, wd, mask, sums[: len(SLOTS)], bias=bd, assignment=ad, recorded=rd, scratch=scratch, xq=xq)
        if two:
            hb.output_error_transposed(xd, wd, t_mask, sums[len(SLOTS):], bias=bd, assignment=tad, scratch=scratch, xq=xq)
        m += int(ch.x.shape[0])
        cast = cast or ch.cast
    torch.cuda.synchronize()
    return sums.cpu().numpy(), m, seen_rec, cast


def rows_from_sums(sums: np.ndarray, m: int, n: int, k: int, formats, map_cand: Optional[MapCandidate], recorded: bool,
                   t_formats=()) -> list[Row]:
    numel_w = float(n * k)
    count = float(m) * float(n)
    rows = []
    for f in formats:
        rows.append(Row(f, FORMAT_BYTES_PER_ELEM[f] * numel_w, *_columns(sums[SLOTS.index(f)], count), tuple(sums[SLOTS.index(f)])))
    for f in t_formats:
        s = sums[len(SLOTS) + SLOTS.index(f)]
        rows.append(Row(f + TRANSPOSE_SUFFIX, FORMAT_BYTES_PER_ELEM[f] * numel_w, *_columns(s, count), tuple(s), {"layout": "transpose"}))
    if map_cand is not None:
        t = map_cand.layout == "transpose"
        s = sums[(len(SLOTS) if t else 0) + SLOTS.index("map")]
        rows.append(Row(map_cand.name, map_cand.tile_bytes, *_columns(s, count), tuple(s), {"layout": "transpose"} if t else {}))
    if recorded:
        s = sums[SLOTS.index("recorded")]
        rows.append(Row("recorded", None, *_columns(s, count), tuple(s)))
    return rows


def evaluate_op(index, op: OpIO, formats, config=None, backend: str = "emulation", chunk_rows: int = 16384,
                x_format: str = "bf16", budgets=(), calib: Optional[OpIO] = None, gptq: bool = False, gptq_damp: float = 0.01,
                transpose: bool = False) -> OpResult:
    """One op of `select_ops` → its rows (or the reason it is skipped).  formats ⊆ SUPPORTED_FORMATS; config: a CompressionConfig
    whose mixed-tile algorithm adds the map candidate (None = pure formats only); x_format: the candidates' activation format.
    budgets: bits per weight, each adding the maps budget:<bits>:output and budget:<bits>:weight (budget_maps.py) chosen on the
    calibration activations `calib` (an OpIO of the same op) and evaluated here, after the other rows; bf16 x_format only.
    gptq: adds, after those, the error-compensated weights (gptq.py) built on `calib` with damp gptq_damp: gptq:<f> for each of bfp8 /
    bfp4 / bfp2 among the formats, gptq:<map name> for the config's map and gptq:budget:<bits>:output for each budget map, each with the
    bytes of its round-to-nearest counterpart; bf16 x_format only.
    transpose: adds <f>+transpose for each of bfp8 / bfp4 / bfp2 among the formats and, with budgets, budget:<bits>:<basis>+transpose
    (implied by a config with the transpose algorithm); a config with "layout": "transpose" gives a map over Wᵀ's grid."""
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {', '.join(BACKENDS)}")
    check_x_format(x_format)
    budgets = tuple(budgets or ())
    if budgets:
        from .budget_maps import check_bits

        if x_format != "bf16":
            raise ValueError("budget maps are chosen and evaluated on bf16 activations: x_format must be bf16")
        for b in budgets:
            check_bits(b)
    if gptq:
        from .gptq import check_damp

        if x_format != "bf16":
            raise ValueError("GPTQ weights are built and evaluated on bf16 activations: x_format must be bf16")
        check_damp(gptq_damp)
    check_layout(config, LAYOUTS)
    transpose = bool(transpose) or (config is not None and config.algorithm == "transpose")
    bad = [f for f in formats if f not in SUPPORTED_FORMATS]
    if bad:
        raise ValueError(f"Unsupported format(s) {bad}. Supported: {', '.join(SUPPORTED_FORMATS)}")
    shape, _ = index.shape_dtype(op.weight)
    res = OpResult(op=op.op, weight=op.weight, shape=tuple(shape), splits=op.splits, x_format=x_format)
    why = check_op(op, tuple(shape))
    if why is not None:
        res.skipped = why
        return res
    n, k = int(shape[0]), int(shape[1])
    if backend == "hip":
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        w = index.load(op.weight, device=dev)
        bias = index.load(op.bias, device=dev) if op.bias else None
    else:
        w = index.load(op.weight)
        bias = index.load(op.bias) if op.bias else None
    if bias is not None and bias.numel() != n:
        res.skipped = f"bias has {bias.numel()} elements, the weight {n} rows"
        return res
    map_cand = search_map(w, config, backend, op.weight)
    map_r = map_cand if map_cand is not None and map_cand.layout == "rows" else None
    map_t = map_cand if map_cand is not None and map_cand.layout == "transpose" else None
    t_formats = [f for f in formats if f in TRANSPOSE_FORMATS] if transpose else []
    it = chunks(op, k, n, chunk_rows)
    if backend == "hip":
        sums, m, seen_rec, cast = hip_sums(it, w, formats, bias, None if map_r is None else map_r.assignment, x_format, t_formats,
                                           None if map_t is None else map_t.assignment)
    else:
        sums, m, seen_rec, cast = emulation_sums(it, w, formats, bias, None if map_r is None else map_r.y, x_format, t_formats,
                                                 None if map_t is None else map_t.y)
    res.m, res.x_cast = m, cast
    res.rows = rows_from_sums(sums, m, n, k, formats, map_cand, seen_rec, t_formats)
    if budgets:
        _budget_rows(res, index, op, w, bias, formats, backend, chunk_rows, budgets, calib, transpose)
    if gptq:
        _gptq_rows(res, op, w, bias, formats, map_cand, backend, chunk_rows, budgets, calib, gptq_damp, transpose)
    return res


def _budget_rows(res: OpResult, index, op: OpIO, w, bias, formats, backend: str, chunk_rows: int, budgets, calib: Optional[OpIO],
                 transpose: bool = False) -> None:
    """Appends the budget maps' rows to res (each map its own LOE pass over the evaluation chunks, the map slot alone), or records in
    res.budget_skipped why a map was not made.  transpose: per budget, the two row-layout maps are followed by their two transposed
    maps, allocated on the transposed tables over Wᵀ's grid."""
    from . import budget_maps as bm

    n, k = res.shape
    layouts = LAYOUTS if transpose else ("rows",)
    names = [(b, layout, basis, bm.map_name(b, basis) + (TRANSPOSE_SUFFIX if layout == "transpose" else ""))
             for b in budgets for layout in layouts for basis in bm.BASES]
    why = "no calibration samples for this op" if calib is None else check_op(calib, (n, k))
    tables = {}
    if why is None:
        res.calib_splits = calib.splits
        cal = chunks(calib, k, n, chunk_rows)
        if backend == "hip":
            h, m_cal = bm.gram_blocks_hip(cal, k, device=w.device)
            if m_cal:
                tables = {layout: bm.tile_error_tables_hip(w, h, layout) for layout in layouts}
        else:
            h, m_cal = bm.gram_blocks_emulation(cal, k)
            if m_cal:
                tables = {layout: bm.tile_error_tables_emulation(w, h, layout) for layout in layouts}
        if not m_cal:
            why = "the calibration samples hold no tokens"
    if why is not None:
        res.budget_skipped.extend((name, why) for _b, _layout, _basis, name in names)
        return
    for b, layout, basis, name in names:
        e_out, e_w = tables[layout]
        t = layout == "transpose"
        got = bm.allocate(e_out if basis == "output" else e_w, formats, b, bm.tiles_hw(k, n) if t else bm.tiles_hw(n, k))
        if isinstance(got, str):
            res.budget_skipped.append((name, got))
            continue
        assignment, _counts, tile_bytes = got
        it = (Chunk(x=ch.x, cast=ch.cast) for ch in chunks(op, k, n, chunk_rows))   # the map slot alone: no recorded output
        if backend == "hip":
            sums, m, _rec, _cast = hip_sums(it, w, [], bias, None if t else assignment, t_assignment=assignment if t else None)
            y = None
        else:
            y = bm.reconstruct_emulation(w, assignment, layout)
            sums, m, _rec, _cast = emulation_sums(it, w, [], bias, None if t else y, map_t_y=y if t else None)
        cand = MapCandidate(name=name, assignment=assignment, y=y, tile_bytes=tile_bytes, layout=layout)
        row = rows_from_sums(sums, m, n, k, [], cand, False)[0]
        row.extra = {"bits": float(b), "basis": basis, "calib_tokens": int(m_cal),
                     "predicted_sse_calib": bm.predicted_sse(e_out, assignment), "assignment": assignment}
        if t:
            row.extra["layout"] = "transpose"
        res.rows.append(row)


def _gptq_outputs(chunk_iter: Iterable, what, bias):
    """Each chunk with Y = X·Ŵᵀ (+ b) as its recorded output, a float32 device tensor: the fused kernel forms R from W as for every row
    and compares it with Y in the recorded slot.  X and Ŵ are bf16 values, so every product is exact in float32 and only the
    accumulation rounds, as in the kernel's own candidates."""
    import torch

    wt = what.T
    for ch in chunk_iter:
        y = ch.x.to(what.device).float() @ wt
        if bias is not None:
            y = y + bias.float().to(what.device)
        yield Chunk(x=ch.x, recorded=y, cast=ch.cast)


def _gptq_rows(res: OpResult, op: OpIO, w, bias, formats, map_cand: Optional[MapCandidate], backend: str, chunk_rows: int, budgets,
               calib: Optional[OpIO], damp: float, transpose: bool = False) -> None:
    """Appends the GPTQ rows to res: one Gram matrix and one host factorisation per op, one sweep and one LOE pass (Ŵ as the weight)
    per candidate; or records in res.budget_skipped why a candidate was not made.  Row layout only: every transposed candidate is
    listed in res.budget_skipped, and no map over Wᵀ's grid reaches a sweep."""
    from . import budget_maps as bm
    from . import gptq as gq

    n, k = res.shape
    row_only = "GPTQ is row-layout only: a transposed candidate has no GPTQ counterpart"
    if transpose:
        res.budget_skipped.extend((f"gptq:{f}{TRANSPOSE_SUFFIX}", row_only) for f in gq.GPTQ_FORMATS if f in formats)
    if map_cand is not None and map_cand.layout != "rows":
        res.budget_skipped.append((f"gptq:{map_cand.name}", row_only))
        map_cand = None
    if transpose:
        res.budget_skipped.extend((f"gptq:{bm.map_name(b, 'output')}{TRANSPOSE_SUFFIX}", row_only) for b in budgets)
    cands = [(f"gptq:{f}", gq.constant_codes(n, k, f), FORMAT_BYTES_PER_ELEM[f] * float(n * k)) for f in gq.GPTQ_FORMATS if f in formats]
    if map_cand is not None:
        cands.append((f"gptq:{map_cand.name}", map_cand.assignment, map_cand.tile_bytes))
    for b in budgets:
        name = bm.map_name(b, "output")
        row = next((r for r in res.rows if r.candidate == name), None)
        if row is not None:
            cands.append((f"gptq:{name}", row.extra["assignment"], row.bytes))
        else:
            res.budget_skipped.append((f"gptq:{name}", f"no {name} map was made"))
    if not cands:
        return
    why = "no calibration samples for this op" if calib is None else check_op(calib, (n, k))
    if why is None:
        res.calib_splits = calib.splits
        cal = chunks(calib, k, n, chunk_rows)
        if backend == "hip":
            h, m_cal = gq.gram_full_hip(cal, k, device=w.device)
            h = h.cpu().numpy()
        else:
            h, m_cal = gq.gram_full_emulation(cal, k)
        why = "the calibration samples hold no tokens" if not m_cal else None
    if why is None:
        u = gq.factor(h, damp)
        if isinstance(u, str):
            why = u
    if why is not None:
        res.budget_skipped.extend((name, why) for name, _codes, _bytes in cands)
        return
    if backend == "hip":
        import torch

        ud = torch.from_numpy(u).to(w.device)
    for name, codes, nbytes in cands:
        it = (Chunk(x=ch.x, cast=ch.cast) for ch in chunks(op, k, n, chunk_rows))   # Ŵ's slot alone: no recorded output
        if backend == "hip":
            what, loss = gq.sweep_hip(w, ud, codes)
            if not bool((what.to(torch.bfloat16).float() == what).all()):
                raise RuntimeError(f"{name}: a GPTQ weight is not a bf16 value, so its products with X are not exact in float32")
            sums, m, _rec, _cast = hip_sums(_gptq_outputs(it, what, bias), w, [], bias)
            s = sums[SLOTS.index("recorded")]
            loss = float(loss.sum())
        else:
            what, loss, _margin = gq.sweep_emulation(w, u, codes)
            sums, m, _rec, _cast = emulation_sums(it, w, [], bias, what)
            s = sums[SLOTS.index("map")]
            loss = float(loss.sum())
        row = Row(name, nbytes, *_columns(s, float(m) * float(n)), tuple(s))
        row.extra = {"damp": float(damp), "calib_tokens": int(m_cal), "calib_loss": loss}
        res.rows.append(row)
