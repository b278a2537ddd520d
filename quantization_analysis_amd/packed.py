"""Packed mixed-tile weights: the bytes a tile map promises, and a linear layer that multiplies with them.

The format is the one include/mtq.h fixes (row layout; tile t = tr * tiles_w + tc of the zero-padded 2-D flatten; blobs of 2048 / 1088 /
576 / 320 bytes for the map codes 0..3; uint32 offsets in units of 64 bytes).  It is this project's own layout, not TTNN's on-device
tile format.

pack_batch / unpack_batch take a batch of equal-shaped tensors and their maps (a search pipeline's resident batch and its results) to one
arena and back with a fixed number of launches; save_dir / load_dir keep a named set of packed tensors in a directory.  linear_grouped /
linear_batch / PackedExperts multiply with every tensor of such an arena (the experts of an MoE layer) over its own rows of X in one
launch; linear_grouped_wide is that product for experts with hundreds of rows (prefill), from the wide-block kernel; as_batch makes the
arena of any list of equal-shaped packed tensors.  glu / glu_grouped are the first half of a gated MLP, act(gate(x)) * up(x), with the
two projections fused in one launch of the wide-block kernel (or, bit for bit the same, unfused); PackedMLP and PackedExpertsMLP are
down(act(gate(x)) * up(x)) as modules, dense and over an arena of experts.

pack_transposed / unpack_transposed / matmul / PackedMatmul close the gap to the transposed layout and to input-major weights without a
new byte format: a transposed-layout map of W (n, k) is a row-layout map of Wᵀ (k, n), so the packed transposed weight IS the ordinary
packed tensor of Wᵀ (shape (k, n), layout "rows"); pack_transposed reads W in place, unpack_transposed writes W's orientation, and
matmul is Y = X·P̂ + b for a packed (k, n) matrix (mtq_packed_matmul: the block kernel's frame over a [k][n] LDS image read with the
transposed LDS read).  A weight stored input-major (y = x @ W) packs with pack() and multiplies with matmul.  matmul(kernel="skinny")
is that product for decode, m <= 32 (mtq_packed_matmul_skinny: the skinny linear kernel's split over K with each tile passed through
a wave-private [k][n] LDS image), and PackedMatmul(kernel="skinny" | "auto") keeps its workspace across calls.

matmul_wide is the (k, n) product above the decode range from the wide-block kernel (mtq_packed_matmul_wide), the block kernel's bits.

pack_batch_transposed / unpack_batch_transposed are pack_transposed / unpack_transposed for a batch of equal-shaped weights
(count, n, k) and the maps of a layout="transpose" search: one arena of ordinary (k, n) tensors, pack_batch's launches and read-back
(mtq_pack_tiles_transposed_batched reads each tile of W by rows through a wave-private LDS image; mtq_unpack_tiles_transposed_batched
writes W's orientation).  scripts/pack_model.py --store-transposed packs a model under a transposed config this way; read_index gives a
directory's index.json, where such a run marks its entries "stored": "transpose".

moe_plan / moe_dispatch / moe_combine / PackedMoE are the rest of an MoE layer around PackedExpertsMLP (csrc/mtq_moe.hip): from the
router's (tokens, top_k) expert ids a stable counting sort on the device gives the grouped entries' row layout (MoEPlan), a row gather
puts the tokens in it, and a weighted un-permute with a fixed summation order brings the experts' rows back; nothing is read back to
the host.  On that staged route the gather and the combine are kernels of their own.
moe_glu / moe_down_combine are the decode route without them (include/mtq_moe_decode.h): the gather inside the grouped skinny GLU
wave's X loads, the combine inside the down projection's reduce, the staged route's bits from five launches for seven and without the
(S, k) and (S, k_out) intermediates; PackedMoE(decode_route="fused") runs plan → moe_glu → moe_down_combine up to decode_max_rows slots.
kernel="chunks" on glu_grouped_skinny, glu_matmul_grouped_skinny, moe_glu and moe_down_combine, and decode_grouped_kernel="chunks" on the
expert MLPs and PackedMoE (include/mtq_glu_chunked.h), give every 32-row chunk of an expert a wave of its own, for routings with hot
experts: the walking kernels' bits, planned on the device.

moe_route / MoERouting / MOE_ROUTINGS are the router in front of that (csrc/mtq_moe_route.hip): from the router GEMM's logits to
(topk_weights, topk_ids) in one launch - softmax or sigmoid scores, a selection-only bias, group-limited top-k, renormalised and scaled
weights - by a rule include/mtq.h pins to the bit on the scores (ties to the lower id); PackedMoE(router=...).forward_logits runs it
and then forward.  The router GEMM stays the model's; the route is not fused into the plan's one-launch kernel.

glu_matmul / glu_matmul_skinny / glu_matmul_grouped / glu_matmul_grouped_skinny are glu and its three variants for packed (k, n) gate and
up matrices (mtq_packed_glu_matmul_wide, _wide_grouped, _skinny, _skinny_grouped: the gated frames with the matmul kernels' feed), bit
for bit two matmul calls into float32 and the combine; PackedMatmulMLP and PackedExpertsMatmulMLP are PackedMLP and PackedExpertsMLP over
such weights, and PackedMoE(stored="transpose") is the layer over them: a pack_model.py --store-transposed directory of an MoE layer's
experts runs with no Python loop over experts.

Not built: a chunked variant of the grouped skinny GLU kernels; pack_transposed of tensors of rank other than 2 (pack_model.py packs
their permuted copies with pack); activations other than ACTS.

Two backends:
  "hip"        the C ABI (csrc/mtq_packed.hip) through hip_backend's wrappers; data lives on the device.
  "emulation"  a NumPy encoder and decoder written from the format's description: the byte-level oracle of the GPU tests, and the way
               the feature works without a GPU.

A map over the transposed layout (params["layout"] = "transpose") is refused by every row-layout entry (pack(layout=...), pack_batch,
as_batch, linear, glu, ...): a group there runs down a column, and the packed format holds row groups only.  pack_transposed is the
entry for such a map, pack_batch_transposed for a batch of them.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import MappingProxyType
from typing import Mapping, Optional

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS, flatten_2d, unflatten_2d
from . import hip_backend as hb
from .hip_backend import PACKED_TILE_BYTES, MtqError

FORMAT_VERSION = 1
TILE = 32
GROUP = 16
_MANT = {1: 7, 2: 3, 3: 1}
BACKENDS = ("hip", "emulation")
KERNELS = ("block", "skinny", "auto")
SKINNY_MAX_M = 32           # include/mtq.h MTQ_PACKED_SKINNY_MAX_M
# kernel="auto" takes the skinny kernel up to this m and the block kernel above it: the largest measured m at which the skinny
# kernel's median is below the block kernel's minimum at every shape and map (profiles/packed_linear_skinny.txt).
AUTO_SKINNY_MAX_M = 32
# kernel="auto" takes the wide-block kernel (linear_wide) from this m on when the library has it; None: never.  The smallest measured m
# from which on the wide kernel's median is below the block kernel's minimum of the same run at every shape and map (DESIGN.md §A.6k,
# profiles/packed_linear_wide.txt).  Both kernels give the same bits, so the gate changes no result.
AUTO_WIDE_MIN_M = 64
MATMUL_KERNELS = ("block", "skinny", "auto")
# matmul(kernel="auto") takes the skinny (k, n) kernel up to this m when the library has it and the block kernel above it; None: never,
# "auto" is "block".  The largest measured m at which, at every shape and map, the skinny kernel's median is below mtq_packed_matmul's
# minimum of the same run by more than that side's own minimum-to-median spread (profiles/packed_matmul_skinny.txt).
AUTO_MATMUL_SKINNY_MAX_M = 32
# matmul(kernel="auto") takes the wide-block (k, n) kernel (matmul_wide) from this m on when the library has it; None: never, "auto" stays
# on the block kernel there.  AUTO_WIDE_MIN_M's rule: the smallest measured m from which on, at every shape and map, the wide median is
# below mtq_packed_matmul's minimum of the same run by more than that side's own minimum-to-median spread (DESIGN.md §A.6t,
# profiles/packed_matmul_wide.txt).  Both kernels give the same bits, so the gate changes no result.
AUTO_MATMUL_WIDE_MIN_M = 64
ACTS =("silu", "none")     # include/mtq.h MTQ_ACT_SILU, MTQ_ACT_NONE
GLU_KERNELS = ("fused", "unfused", "auto")
GLU_GROUPED_KERNELS = ("fused", "unfused")
MLP_DECODE_KERNELS = ("pair", "fused")   # PackedMLP(decode_kernel=...): glu(kernel="auto")'s five launches at m <= 32, or glu_skinny's two
# glu(kernel="auto") above the skinny range takes the fused kernel (mtq_packed_glu_wide) from this m on; None: never, "auto" stays
# unfused there.  The rule of AUTO_WIDE_MIN_M: the smallest measured m from which on the fused median is below the unfused minimum of the
# same run at every shape and map (profiles/packed_glu.txt).  Both routes give the same bits, so the gate changes no
# result.
AUTO_GLU_FUSED_MIN_M = 64
# glu_matmul(kernel="auto"), the same two gates for (k, n) weights, constants of their own: two matmul(kernel="skinny") calls and the
# combine up to AUTO_GLU_MATMUL_SKINNY_MAX_M, the fused kernel (mtq_packed_glu_matmul_wide) from AUTO_GLU_MATMUL_FUSED_MIN_M on (None:
# never), "unfused" between.  They start at the linear family's values; DESIGN.md §A.6x and profiles/packed_glu_matmul.txt have the
# measurement that keeps or moves them.  All routes above the skinny range give the same bits, so the upper gate changes no result.
AUTO_GLU_MATMUL_SKINNY_MAX_M = 32
AUTO_GLU_MATMUL_FUSED_MIN_M = 64
MATMUL_MLP_DECODE_KERNELS = ("pair", "fused")   # PackedMatmulMLP(decode_kernel=...): as MLP_DECODE_KERNELS, with glu_matmul / glu_matmul_skinny
MOE_STORED = ("rows", "transpose")              # PackedMoE(stored=...): the index.json word of a pack_model directory
# The largest error of the device's silu (csrc/mtq_glu.hpp glu_value at u = 1) against float64, in units of 2^-24 relative to the value,
# over every 2^10-th float32 of [-88.7228, 100], rounded up to a hundredth: measured; the GPU tests hold the kernel to
# it and form their bound's constant from it.  Below -88.7228 expf(-g) overflows and the sequence gives -0.
GLU_SILU_MAX_ULPS = 2.43
# A bound on |silu'| (its maximum is 1.09984 near g = 2.4): the slope the accuracy bound of glu's tests multiplies the gate's error by.
GLU_SILU_SLOPE_MAX = 1.1


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def offsets_of(amap) -> np.ndarray:
    """uint32[tiles + 1]: the exclusive prefix sum of the blob sizes, in units of 64 bytes."""
    a = np.asarray(amap, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 3):
        raise MtqError("map codes must be MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
    units = np.concatenate([[0], np.cumsum(np.asarray(PACKED_TILE_BYTES, dtype=np.int64)[a] // 64)])
    if units[-1] > 0xFFFFFFFF:
        raise MtqError("the stream is too long for 32-bit offsets in units of 64 bytes")
    return units.astype(np.uint32)


@dataclass
class PackedTensor:
    """A tensor in the packed mixed-tile format.  shape / shape_info: the original tensor and its 2-D flatten (tile_utils.flatten_2d);
    rows, cols: the flatten's sides; map: int8 (tiles_h, tiles_w); offsets: uint32 [tiles + 1]; data: the uint8 stream, a NumPy array or
    a device tensor."""

    shape: tuple
    shape_info: tuple
    rows: int
    cols: int
    map: np.ndarray
    offsets: np.ndarray
    data: object
    layout: str = "rows"
    _tables: object = None      # hip: the device copies of map and offsets (hip_backend.PackedTables), made on first use
    _batch: object = None       # (PackedBatch, index) of a tensor pack_batch made: its data is a slice of the batch's arena

    @property
    def nbytes(self) -> int:
        """Bytes of the stream."""
        return int(self.offsets[-1]) * 64

    @property
    def total_bytes(self) -> int:
        """The stream plus what it takes to find a tile in it: the map (1 B per tile) and the offsets (4 B per tile + 4)."""
        return self.nbytes + int(self.map.size) + 4 * int(self.offsets.size)

    @property
    def on_device(self) -> bool:
        return _is_torch(self.data) and bool(self.data.is_cuda)

    def counts(self) -> dict:
        c = np.bincount(self.map.reshape(-1).astype(np.int64), minlength=4)
        return {f: int(c[i]) for i, f in enumerate(MIXED_TILE_FORMATS)}

    def tables(self):
        if self._tables is None:
            self._tables = hb.PackedTables.on_device(self.map, self.offsets, self.data.device if self.on_device else None)
        return self._tables


def check_layout(layout: str) -> None:
    """Raises for every layout but "rows": the packed format holds row groups only."""
    if layout != "rows":
        raise MtqError(f"the packed format holds the row layout only; a map over layout {layout!r} cannot be packed")


_check_layout = check_layout


def _check_map(amap, rows: int, cols: int) -> np.ndarray:
    th, tw = -(-rows // TILE), -(-cols // TILE)
    a = np.asarray(amap)
    if a.size != th * tw:
        raise MtqError(f"assignment has {a.size} entries, tensor has {th}x{tw} tiles")
    a = np.ascontiguousarray(a.astype(np.int8).reshape(th, tw))
    if a.min() < 0 or a.max() > 3:
        raise MtqError("map codes must be MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
    return a


# ----------------------------------------------------------------------------- the NumPy encoder and decoder

def bf16_round_bits(u: np.ndarray) -> np.ndarray:
    """Round to nearest even on the raw word (uint32 wrap, no NaN case), low half cleared."""
    return (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)


def encode_groups(u: np.ndarray, mant: int) -> tuple[np.ndarray, np.ndarray]:
    """uint32 words [..., 16] → (shared exponent uint8 [...], codes uint8 [..., 16]); code = (sign << mant) | man."""
    e = (u >> np.uint32(23)) & np.uint32(0xFF)
    shared = e.max(axis=-1, keepdims=True)
    d = (shared - e).astype(np.uint64)
    man = ((u & np.uint32(0x7FFFFF)) | np.uint32(1 << 23)).astype(np.uint64)
    man = np.where(d > 31, np.uint64(0), man >> np.minimum(d, np.uint64(31))).astype(np.uint32)
    shift = 24 - mant
    rv = man & np.uint32((1 << shift) - 1)
    tie = np.uint32(1 << (shift - 1))
    man = man >> np.uint32(shift)
    up = (rv > tie) | ((rv == tie) & ((man & np.uint32(1)) == 1))
    man = np.minimum(man + up.astype(np.uint32), np.uint32((1 << mant) - 1))      # saturating round-up
    man = np.where(e == 0, np.uint32(0), man)                                       # zero / denormal input
    sign = np.where(man == 0, np.uint32(0), u >> np.uint32(31))
    return shared[..., 0].astype(np.uint8), ((sign << np.uint32(mant)) | man).astype(np.uint8)


def decode_groups(shared: np.ndarray, codes: np.ndarray, mant: int) -> np.ndarray:
    """The inverse: (uint8 [...], uint8 [..., 16]) → the float32 words the quantizer writes, uint32 [..., 16]."""
    c = codes.astype(np.uint32)
    sh = shared.astype(np.uint32)[..., None]
    qmax = np.uint32((1 << mant) - 1)
    man = c & qmax
    sign = c >> np.uint32(mant)
    msb = np.zeros_like(man)
    for b in range(mant):
        msb = np.where((man >> np.uint32(b)) & np.uint32(1) == 1, np.uint32(b), msb)
    sc = np.uint32(mant - 1) - msb
    ms = (man << (sc + np.uint32(1))) & qmax
    exp_out = sh - sc                                                               # wraps below sc, kept
    bits = (sign << np.uint32(31)) | (exp_out << np.uint32(23)) | (ms << np.uint32(23 - mant))
    return np.where(man == 0, np.uint32(0), bits).astype(np.uint32)


def _tiles_u32(x2d: np.ndarray) -> tuple[np.ndarray, int, int]:
    """float32 (rows, cols) → uint32 [tiles, 64 groups, 16] of the zero-padded matrix."""
    rows, cols = x2d.shape
    th, tw = -(-rows // TILE), -(-cols // TILE)
    pad = np.zeros((th * TILE, tw * TILE), dtype=np.uint32)
    pad[:rows, :cols] = np.ascontiguousarray(x2d, dtype=np.float32).view(np.uint32)
    return pad.reshape(th, TILE, tw, TILE).transpose(0, 2, 1, 3).reshape(th * tw, 2 * TILE, GROUP), th, tw


def _pack_bits(codes: np.ndarray, bits: int) -> np.ndarray:
    """uint8 codes [T, 1024] of `bits` bits each → bytes, element e at bits `bits` * (e % (8 / bits))."""
    per = 8 // bits
    c = codes.reshape(codes.shape[0], -1, per).astype(np.uint8)
    out = np.zeros(c.shape[:2], dtype=np.uint8)
    for j in range(per):
        out |= c[:, :, j] << np.uint8(bits * j)
    return out


def _unpack_bits(raw: np.ndarray, bits: int) -> np.ndarray:
    per = 8 // bits
    out = np.empty(raw.shape + (per,), dtype=np.uint8)
    for j in range(per):
        out[..., j] = (raw >> np.uint8(bits * j)) & np.uint8((1 << bits) - 1)
    return out.reshape(raw.shape[0], -1)


def encode(x2d: np.ndarray, amap: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """float32 (rows, cols) and its int8 (tiles_h, tiles_w) map → (stream uint8, offsets uint32)."""
    g, th, tw = _tiles_u32(x2d)
    a = amap.reshape(-1)
    offsets = offsets_of(a)
    data = np.zeros(int(offsets[-1]) * 64, dtype=np.uint8)
    start = offsets[:-1].astype(np.int64) * 64
    for f in range(4):
        sel = np.flatnonzero(a == f)
        if sel.size == 0:
            continue
        size = PACKED_TILE_BYTES[f]
        if f == 0:
            blobs = (bf16_round_bits(g[sel]) >> np.uint32(16)).astype("<u2").reshape(sel.size, -1).view(np.uint8)
        else:
            shared, codes = encode_groups(g[sel], _MANT[f])
            blobs = np.concatenate([shared, _pack_bits(codes.reshape(sel.size, -1), _MANT[f] + 1)], axis=1)
        assert blobs.shape == (sel.size, size)
        data[(start[sel][:, None] + np.arange(size)[None, :]).reshape(-1)] = blobs.reshape(-1)
    return data, offsets


def decode(data: np.ndarray, amap: np.ndarray, offsets: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """The stream → uint32 words of the (rows, cols) float32 tensor the map's quantisation writes."""
    th, tw = amap.shape
    a = amap.reshape(-1)
    start = np.asarray(offsets[:-1], dtype=np.int64) * 64
    tiles = np.zeros((th * tw, 2 * TILE, GROUP), dtype=np.uint32)
    for f in range(4):
        sel = np.flatnonzero(a == f)
        if sel.size == 0:
            continue
        size = PACKED_TILE_BYTES[f]
        blobs = data[(start[sel][:, None] + np.arange(size)[None, :])]
        if f == 0:
            tiles[sel] = (np.ascontiguousarray(blobs).view("<u2").astype(np.uint32) << np.uint32(16)).reshape(sel.size, 2 * TILE, GROUP)
        else:
            codes = _unpack_bits(blobs[:, 64:], _MANT[f] + 1).reshape(sel.size, 2 * TILE, GROUP)
            tiles[sel] = decode_groups(blobs[:, :64], codes, _MANT[f])
    pad = tiles.reshape(th, tw, TILE, TILE).transpose(0, 2, 1, 3).reshape(th * TILE, tw * TILE)
    return np.ascontiguousarray(pad[:rows, :cols])


# ----------------------------------------------------------------------------- the public functions

def pack(x, amap, backend: str = "emulation", layout: str = "rows") -> PackedTensor:
    """x (NumPy array or torch tensor of any rank; bf16 and float32 storage are packed as they are, anything else as float32) under the
    int8 tile map `amap` of its 2-D flatten → PackedTensor.  hip: the stream stays on the device."""
    _check_layout(layout)
    _check_backend(backend)
    if backend == "hip":
        hb.require_gpu()
        shape = tuple(x.shape) if hasattr(x, "shape") else ()
        x2d, info = hb.to_device_2d(x)
        rows, cols = (int(v) for v in x2d.shape)
        a = _check_map(amap, rows, cols)
        tables = hb.PackedTables.on_device(a, device=x2d.device)
        data = hb.pack_tiles(x2d, tables)
        return PackedTensor(shape, info, rows, cols, a, offsets_of(a), data, _tables=tables)
    xf = x.detach().to("cpu").float().numpy() if _is_torch(x) else np.asarray(x, dtype=np.float32)
    x2d, info = flatten_2d(xf)
    rows, cols = x2d.shape
    a = _check_map(amap, rows, cols)
    data, offsets = encode(x2d, a)
    return PackedTensor(tuple(xf.shape), info, rows, cols, a, offsets, data)


def _host_data(pt: PackedTensor) -> np.ndarray:
    d = pt.data.cpu().numpy() if _is_torch(pt.data) else np.asarray(pt.data, dtype=np.uint8)
    if d.size < pt.nbytes:
        raise MtqError(f"the stream holds {d.size} bytes, its offsets say {pt.nbytes}")
    return d


def _device_data(pt: PackedTensor):
    import torch

    if not pt.on_device:
        pt.data = torch.from_numpy(np.ascontiguousarray(_host_data(pt))).to(torch.device("cuda", torch.cuda.current_device()))
        pt._tables = None
    return pt.data


def unpack(pt: PackedTensor, backend: str = "emulation", dtype: str = "float32"):
    """The tensor the map's quantisation writes, in the original shape.  dtype "float32": bit for bit the reconstruction (K3);
    "bfloat16": the same values as bf16, which is exact.  emulation → NumPy float32, or a torch CPU bfloat16 tensor; hip → device tensor."""
    _check_layout(pt.layout)
    _check_out_dtype(dtype, "dtype")
    if backend == "hip":
        import torch

        hb.require_gpu()
        y = hb.unpack_tiles(_device_data(pt), pt.tables(), pt.rows, pt.cols, _torch_dtype(dtype))
        return hb.unflatten(y, pt.shape_info)
    _check_backend(backend)
    bits = decode(_host_data(pt), pt.map, pt.offsets, pt.rows, pt.cols)
    if dtype == "float32":
        y = unflatten_2d(bits.view(np.float32), pt.shape_info)
        return y
    import torch

    half = torch.from_numpy((bits >> np.uint32(16)).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    kind, v = pt.shape_info
    return half.reshape(()) if kind == "scalar" else (half.reshape(-1)[:v] if kind == "vector" else half.reshape(tuple(v)))


# ----------------------------------------------------------------------------- the two orientations of a packed operand

@dataclass(frozen=True)
class _Orientation:
    """What differs between the products with a packed (n, k) weight (linear, glu, PackedLinear, ...) and those with a packed (k, n)
    matrix (matmul, glu_matmul, PackedMatmul, ...).  Every shared body below takes one of the two instances, _NK or _KN, first.  Apart
    from the reading of (n, k) and the emulation's product it holds NAMES - of hip_backend's bindings, predicates and symbol tuples,
    and of this module's constants, public functions and _need_* checks - which a body looks up when it runs (getattr(hb, name),
    globals()[name]): replacing one of them by module attribute takes effect at the next call, as it always did.  A rule that holds
    for one orientation only is a field here, not a test of the family inside a body."""

    kn: bool                        # the operand is a (k, n) matrix: (n, k) = (cols, rows), the product x @ w; else (rows, cols), x @ w.T
    noun: str                       # what messages call the operand
    rank2: str                      # the refusal of an operand that is not 2-D; {what} is the caller's name
    pair_rank2: str                 # the same for one of a gate / up pair
    down_shape: str                 # a down projection's shape in messages
    kernel_before_rank: bool        # a bad `kernel` is reported before a bad rank
    # this module's constants
    kernels: str
    auto_skinny_max_m: str
    auto_wide_min_m: str
    skinny_gates_may_be_none: bool  # None in a *_SKINNY_MAX_M constant means never; else it is compared as it is
    grouped_kernels: str
    grouped_auto_kernel: str
    glu_auto_skinny_max_m: str
    glu_auto_fused_min_m: str
    mlp_decode_kernels: str
    # this module's public functions
    product: str
    grouped: str
    grouped_wide: str
    glu: str
    glu_skinny: str
    glu_grouped: str
    glu_grouped_skinny: str
    # hip_backend's bindings and predicates
    hb_block: str
    hb_wide: str
    hb_skinny: str
    hb_skinny_size: str
    has_auto_skinny: Optional[str]  # what "auto" asks before it takes the skinny binding; None: nothing
    has_auto_wide: str              # and before it takes the wide one
    hb_grouped: Mapping             # resolved grouped kernel → (binding, size function, predicate or None, who needs it, symbols, hint)
    hb_glu_fused: str
    hb_glu_skinny: str
    hb_glu_grouped_fused: str
    hb_glu_grouped_fused_size: str
    hb_glu_grouped_skinny: str
    hb_glu_grouped_skinny_size: str
    # the _need_* checks (hb, what) a hip call makes, by role; () where a call asks for no optional symbol
    need_product: tuple
    need_skinny: tuple
    need_wide: tuple
    need_glu: tuple
    need_glu_auto_skinny: tuple
    need_glu_skinny: tuple
    need_glu_grouped: tuple
    # the module classes
    module_size_every_m: bool       # the dense module's workspace is the maximum over m = 1 .. 32 and needs no predicate; else it is
    #                                 sized at m = 32 alone, when has_auto_skinny holds
    module_needs: tuple             # what the dense module's constructor asks for on hip
    experts_keep_size: bool         # the experts module keeps the size function it found in its constructor
    experts_wide_lacks: Optional[tuple]   # (who, hint) of its refusal of wide_min_rows on a library without the wide kernel; None: hb_grouped's
    experts_mlp_wide_last: bool     # the experts MLP looks for the wide grouped kernel after the gated ones, and words the refusal itself

    def n_k(self, t):
        """(n, k) of a PackedTensor or PackedBatch."""
        return (t.cols, t.rows) if self.kn else (t.rows, t.cols)

    def times(self, x64, w64):
        """The emulation's product with the decoded (rows, cols) operand."""
        return x64 @ w64 if self.kn else x64 @ w64.T


_LACKS = "which this build of libmtq_hip.so lacks: rebuild it from this tree"

_NK = _Orientation(
    kn=False, noun="weight", rank2="{what} needs a 2-D (n, k) weight, the packed tensor is {shape}",
    pair_rank2="glu needs 2-D (n, k) weights, the packed {name} tensor is {shape}", down_shape="(k_out, {n})", kernel_before_rank=True,
    kernels="KERNELS", auto_skinny_max_m="AUTO_SKINNY_MAX_M", auto_wide_min_m="AUTO_WIDE_MIN_M", skinny_gates_may_be_none=False,
    grouped_kernels="GROUPED_KERNELS", grouped_auto_kernel="GROUPED_AUTO_KERNEL", glu_auto_skinny_max_m="AUTO_SKINNY_MAX_M",
    glu_auto_fused_min_m="AUTO_GLU_FUSED_MIN_M", mlp_decode_kernels="MLP_DECODE_KERNELS",
    product="linear", grouped="linear_grouped", grouped_wide="linear_grouped_wide", glu="glu", glu_skinny="glu_skinny",
    glu_grouped="glu_grouped", glu_grouped_skinny="glu_grouped_skinny",
    hb_block="packed_linear", hb_wide="packed_linear_wide", hb_skinny="packed_linear_skinny", hb_skinny_size="packed_linear_skinny_workspace_bytes",
    has_auto_skinny=None, has_auto_wide="has_packed_linear_wide",
    hb_grouped=MappingProxyType({
        # "walk" asks for nothing: its binding is looked up by name, as before there was a choice
        "walk": ("packed_linear_skinny_grouped", "packed_linear_skinny_grouped_workspace_bytes", None, None, None, None),
        "chunks": ("packed_linear_skinny_grouped_chunked", "packed_linear_skinny_grouped_chunked_workspace_bytes", "has_packed_linear_grouped_chunked",
                   'kernel="chunks"', "mtq_packed_linear_skinny_grouped_chunked", ', or use kernel="walk"'),
        "wide": ("packed_linear_wide_grouped", "packed_linear_wide_grouped_workspace_bytes", "has_packed_linear_wide_grouped",
                 "linear_grouped_wide", "mtq_packed_linear_wide_grouped", ", or use linear_grouped")}),
    hb_glu_fused="packed_glu_wide", hb_glu_skinny="packed_glu_skinny", hb_glu_grouped_fused="packed_glu_wide_grouped",
    hb_glu_grouped_fused_size="packed_glu_wide_grouped_workspace_bytes", hb_glu_grouped_skinny="packed_glu_skinny_grouped",
    hb_glu_grouped_skinny_size="packed_glu_skinny_grouped_workspace_bytes",
    need_product=(), need_skinny=(), need_wide=(), need_glu=("_need_glu",), need_glu_auto_skinny=(), need_glu_skinny=("_need_glu_skinny",),
    need_glu_grouped=("_need_glu",),
    module_size_every_m=True, module_needs=(), experts_keep_size=False, experts_wide_lacks=("wide_min_rows", ", or leave wide_min_rows None"),
    experts_mlp_wide_last=True)

_KN = _Orientation(
    kn=True, noun="matrix", rank2="{what} needs a 2-D packed (k, n) matrix, the packed tensor is {shape}",
    pair_rank2="{what} needs a 2-D packed (k, n) matrix, the packed tensor is {shape}", down_shape="({n}, k_out)", kernel_before_rank=False,
    kernels="MATMUL_KERNELS", auto_skinny_max_m="AUTO_MATMUL_SKINNY_MAX_M", auto_wide_min_m="AUTO_MATMUL_WIDE_MIN_M", skinny_gates_may_be_none=True,
    grouped_kernels="MATMUL_GROUPED_KERNELS", grouped_auto_kernel="MATMUL_GROUPED_AUTO_KERNEL",
    glu_auto_skinny_max_m="AUTO_GLU_MATMUL_SKINNY_MAX_M", glu_auto_fused_min_m="AUTO_GLU_MATMUL_FUSED_MIN_M",
    mlp_decode_kernels="MATMUL_MLP_DECODE_KERNELS",
    product="matmul", grouped="matmul_grouped", grouped_wide="matmul_grouped_wide", glu="glu_matmul", glu_skinny="glu_matmul_skinny",
    glu_grouped="glu_matmul_grouped", glu_grouped_skinny="glu_matmul_grouped_skinny",
    hb_block="packed_matmul", hb_wide="packed_matmul_wide", hb_skinny="packed_matmul_skinny", hb_skinny_size="packed_matmul_skinny_workspace_bytes",
    has_auto_skinny="has_packed_matmul_skinny", has_auto_wide="has_packed_matmul_wide",
    hb_grouped=MappingProxyType({   # every kernel is asked for, and the refusal names hip_backend's tuple of its symbols
        "walk": ("packed_matmul_skinny_grouped", "packed_matmul_skinny_grouped_workspace_bytes", "has_packed_matmul_grouped",
                 'matmul_grouped(kernel="walk")', "MATMUL_GROUPED", ""),
        "chunks": ("packed_matmul_skinny_grouped_chunked", "packed_matmul_skinny_grouped_chunked_workspace_bytes", "has_packed_matmul_grouped_chunked",
                   'matmul_grouped(kernel="chunks")', "MATMUL_GROUPED_CHUNKED", ""),
        "wide": ("packed_matmul_wide_grouped", "packed_matmul_wide_grouped_workspace_bytes", "has_packed_matmul_wide_grouped",
                 "matmul_grouped_wide", "MATMUL_WIDE_GROUPED", "")}),
    hb_glu_fused="packed_glu_matmul_wide", hb_glu_skinny="packed_glu_matmul_skinny", hb_glu_grouped_fused="packed_glu_matmul_wide_grouped",
    hb_glu_grouped_fused_size="packed_glu_matmul_wide_grouped_workspace_bytes", hb_glu_grouped_skinny="packed_glu_matmul_skinny_grouped",
    hb_glu_grouped_skinny_size="packed_glu_matmul_skinny_grouped_workspace_bytes",
    need_product=("_need_matmul",), need_skinny=("_need_matmul_skinny",), need_wide=("_need_matmul_wide",),
    need_glu=("_need_matmul", "_need_glu_matmul"), need_glu_auto_skinny=("_need_matmul_skinny",), need_glu_skinny=("_need_glu_matmul_skinny",),
    need_glu_grouped=("_need_glu_matmul",),
    module_size_every_m=False, module_needs=("_need_matmul",), experts_keep_size=True, experts_wide_lacks=None, experts_mlp_wide_last=False)


def _needs(names, hb, what: str) -> None:
    """The _need_* checks `names` of this module, in order: the first optional symbols the library lacks raise, named, for `what`."""
    for name in names:
        globals()[name](hb, what)


def _check_kernel(kernel, kernels) -> None:
    if kernel not in kernels:
        raise MtqError(f"kernel must be one of {kernels}, got {kernel!r}")


def _check_backend(backend) -> None:
    if backend not in BACKENDS:
        raise MtqError(f"backend must be one of {BACKENDS}, got {backend!r}")


def _check_out_dtype(out_dtype, name: str = "out_dtype") -> None:
    if out_dtype not in ("float32", "bfloat16"):
        raise MtqError(f"{name} must be 'float32' or 'bfloat16', got {out_dtype!r}")


def _torch_dtype(out_dtype: str):
    import torch

    return torch.float32 if out_dtype == "float32" else torch.bfloat16


def _check_rank2(o: _Orientation, pt: PackedTensor, what: str) -> None:
    _check_layout(pt.layout)
    if len(pt.shape) != 2:
        raise MtqError(o.rank2.format(what=what, shape=pt.shape))


def _check_pair(o: _Orientation, gate: PackedTensor, up: PackedTensor, what: str) -> None:
    for name, pt in (("gate", gate), ("up", up)):
        _check_layout(pt.layout)
        if len(pt.shape) != 2:
            raise MtqError(o.pair_rank2.format(what=what, name=name, shape=pt.shape))
    if (gate.rows, gate.cols) != (up.rows, up.cols):
        raise MtqError(f"gate and up must have one shape, got {gate.rows}x{gate.cols} and {up.rows}x{up.cols}")


def _host_f32(x) -> np.ndarray:
    return x.detach().to("cpu").float().numpy() if _is_torch(x) else np.asarray(x, dtype=np.float32)


def _host_f64(v, shape=None, name: str = ""):
    """A bias on the host in float64, or None; held to `shape` when one is given."""
    if v is None:
        return None
    b = v.detach().to("cpu").double().numpy() if _is_torch(v) else np.asarray(v, dtype=np.float64)
    if shape is not None and b.shape != shape:
        raise MtqError(f"{name} must be {shape}, got {b.shape}")
    return b


def _round_out(h64: np.ndarray, out_dtype: str):
    """float64 → float32 once, and from there to bf16: the emulation's one rounding."""
    with np.errstate(over="ignore"):
        y32 = h64.astype(np.float32)
    if out_dtype == "float32":
        return y32
    import torch

    return torch.from_numpy(y32).to(torch.bfloat16)


def _at_most(o: _Orientation, name: str, m: int) -> bool:
    """m <= the *_SKINNY_MAX_M constant `name` of this module."""
    gate = globals()[name]
    return (gate is not None or not o.skinny_gates_may_be_none) and m <= gate


def _takes_skinny(o: _Orientation, hb, what: str, kernel: str, m: int) -> bool:
    """Whether `kernel` means the skinny binding at this m: "skinny" always (what it needs is asked for, and no other kernel stands in),
    "auto" up to the orientation's constant, on a library that has what the orientation asks for."""
    if kernel == "skinny":
        if m > SKINNY_MAX_M:
            raise MtqError(f'kernel="skinny" takes m <= {SKINNY_MAX_M}, got m = {m}')
        _needs(o.need_skinny, hb, f'{what}(kernel="skinny")')
        return True
    return kernel == "auto" and _at_most(o, o.auto_skinny_max_m, m) and (o.has_auto_skinny is None or getattr(hb, o.has_auto_skinny)())


def _product(o: _Orientation, what: str, x, pt: PackedTensor, bias, out_dtype, backend, kernel, split, workspace):
    """linear and matmul."""
    _check_layout(pt.layout)
    if o.kernel_before_rank:
        _check_kernel(kernel, globals()[o.kernels])
    if len(pt.shape) != 2:
        raise MtqError(o.rank2.format(what=what, shape=pt.shape))
    if not o.kernel_before_rank:
        _check_kernel(kernel, globals()[o.kernels])
    backend = backend or ("hip" if pt.on_device else "emulation")
    _check_out_dtype(out_dtype)
    n, k = o.n_k(pt)
    if backend == "hip":
        if x.dim() != 2 or x.shape[1] != k:
            raise MtqError(f"x must be (m, {k}), got {tuple(x.shape)}")
        _needs(o.need_product, hb, what)
        dtype = _torch_dtype(out_dtype)
        m = int(x.shape[0])
        if _takes_skinny(o, hb, what, kernel, m):
            return getattr(hb, o.hb_skinny)(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=dtype, split=split, workspace=workspace)
        wide_min_m = globals()[o.auto_wide_min_m]
        if kernel == "auto" and wide_min_m is not None and m >= wide_min_m and getattr(hb, o.has_auto_wide)():
            return getattr(hb, o.hb_wide)(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=dtype)
        return getattr(hb, o.hb_block)(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=dtype)
    _check_backend(backend)
    xf = _host_f32(x)
    if xf.ndim != 2 or xf.shape[1] != k:
        raise MtqError(f"x must be (m, {k}), got {xf.shape}")
    w = decode(_host_data(pt), pt.map, pt.offsets, pt.rows, pt.cols).view(np.float32)
    y = o.times(xf.astype(np.float64), w.astype(np.float64))
    if bias is not None:
        y = y + _host_f64(bias)[None, :]
    return _round_out(y, out_dtype)


def _product_wide(o: _Orientation, what: str, x, pt: PackedTensor, bias, out_dtype, backend):
    """linear_wide and matmul_wide."""
    _check_rank2(o, pt, what)
    backend = backend or ("hip" if pt.on_device else "emulation")
    _check_out_dtype(out_dtype)
    if backend != "hip":
        return globals()[o.product](x, pt, bias=bias, out_dtype=out_dtype, backend=backend)
    n, k = o.n_k(pt)
    if x.dim() != 2 or x.shape[1] != k:
        raise MtqError(f"x must be (m, {k}), got {tuple(x.shape)}")
    _needs(o.need_wide, hb, what)
    return getattr(hb, o.hb_wide)(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=_torch_dtype(out_dtype))


def linear(x, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, kernel: str = "block", split: int = 0,
           workspace=None):
    """Y = X·Ŵᵀ + b with the packed (n, k) weight `pt` (nn.Linear convention).  hip (the default when the stream is on the device):
    X an (m, k) bf16 device tensor, bias float32, through mtq_packed_linear.  emulation: the float64 product of the unpacked weight,
    rounded once to float32 (or from there to bf16) — the reference the GPU tests hold the kernel to, not a fast path.

    kernel: "block" (the default; any m), "skinny" (the split-K kernel for decode, m <= 32; `split` slices of K, 0 = the library's
    choice, and an optional uint8 device `workspace` of hip_backend.packed_linear_skinny_workspace_bytes bytes) or "auto" (skinny for
    m <= AUTO_SKINNY_MAX_M, block above; from m = AUTO_WIDE_MIN_M on, when that is not None and the library has it, the wide-block
    kernel of linear_wide, whose bits are the block kernel's).  The skinny and the block kernel sum in different orders: each is
    bit-stable, they may differ in the last bits.  The emulation computes the same float64 product under all three names."""
    return _product(_NK, "linear", x, pt, bias, out_dtype, backend, kernel, split, workspace)


def linear_wide(x, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None):
    """linear(kernel="block")'s product and, on hip, its bits, through mtq_packed_linear_wide: the wide-block kernel for m above the
    decode range (prefill), 128 x 128 outputs to a workgroup, whose waves decode whole tiles of the weight.  Correct for any m
    (m = 0 gives (0, n)); faster than the block kernel from m = 64 on, the smallest m measured.  A library without the symbol raises MtqError: there is no
    fall-back to the block kernel here (linear(kernel="auto") is the call that chooses).  emulation: linear's float64 product."""
    return _product_wide(_NK, "linear", x, pt, bias, out_dtype, backend)


# ----------------------------------------------------------------------------- the transposed layout and (k, n) weights

def _need_matmul(hb, what: str) -> None:
    if not hb.has_packed_matmul():
        raise MtqError(f"{what} needs mtq_pack_tiles_transposed, mtq_unpack_tiles_transposed and mtq_packed_matmul, which this build of "
                       "libmtq_hip.so lacks: rebuild it from this tree")


def _need_matmul_wide(hb, what: str) -> None:
    if not hb.has_packed_matmul_wide():
        raise MtqError(f"{what} needs mtq_packed_matmul_wide, {_LACKS}")


def _check_kn(pt: PackedTensor, what: str) -> None:
    _check_rank2(_KN, pt, what)


def pack_transposed(w, amap, backend: str = "emulation") -> PackedTensor:
    """The packed TRANSPOSE of the 2-D weight w (n, k) under a map over Wᵀ's tile grid ceil(k/32) × ceil(n/32) - what a mixed-tile
    search with params["layout"] = "transpose" (or layer_output_error.py's budget_<B>_<basis>_transpose.npy) writes for W.  The result
    is an ordinary PackedTensor of shape (k, n) in the row layout: save / load, unpack (which gives Wᵀ) and matmul take it as it is.
    hip: w is read in place through mtq_pack_tiles_transposed (no transposed copy).  emulation: pack(np.ascontiguousarray(w.T), amap)."""
    _check_backend(backend)
    if len(tuple(w.shape)) != 2 or 0 in tuple(w.shape):
        raise MtqError(f"pack_transposed takes a non-empty 2-D (n, k) weight, got {tuple(w.shape)}")
    n, k = (int(v) for v in w.shape)
    a = _check_map(amap, k, n)
    if np.ndim(amap) == 2 and tuple(np.shape(amap)) != a.shape:
        raise MtqError(f"the map is {'x'.join(map(str, np.shape(amap)))} tiles, the transposed weight has {a.shape[0]}x{a.shape[1]}: "
                       "pack_transposed takes a map over the transpose's grid")
    if backend == "hip":
        import torch

        _need_matmul(hb, "pack_transposed")
        hb.require_gpu()
        if _is_torch(w) and w.is_cuda and w.dtype in (torch.bfloat16, torch.float32) and w.stride(-1) == 1:
            w2d = w                                  # a device view with contiguous rows is read in place, whatever its pitch
        else:
            w2d, _info = hb.to_device_2d(w)
        tables = hb.PackedTables.on_device(a, device=w2d.device)
        data = hb.pack_tiles_transposed(w2d, tables)
        return PackedTensor((k, n), ("nd", (k, n)), k, n, a, offsets_of(a), data, _tables=tables)
    wf = w.detach().to("cpu").float().numpy() if _is_torch(w) else np.asarray(w, dtype=np.float32)
    return pack(np.ascontiguousarray(wf.T), a)


def unpack_transposed(pt: PackedTensor, backend: str = "emulation", dtype: str = "float32"):
    """The (n, k) weight whose packed transpose `pt` (shape (k, n)) is: unpack(pt) transposed, written in W's orientation.  float32: bit
    for bit what K3T (mtq_apply_assignment_transposed) and scripts/reconstruct_mixed_tile_assignment.py --layout transpose give for W
    and the map; bfloat16: the same values, exact.  hip: mtq_unpack_tiles_transposed, a device tensor."""
    _check_kn(pt, "unpack_transposed")
    _check_out_dtype(dtype, "dtype")
    if backend == "hip":
        _need_matmul(hb, "unpack_transposed")
        hb.require_gpu()
        return hb.unpack_tiles_transposed(_device_data(pt), pt.tables(), pt.cols, pt.rows, _torch_dtype(dtype))
    _check_backend(backend)
    y = unpack(pt, backend="emulation", dtype=dtype)
    return y.t().contiguous() if _is_torch(y) else np.ascontiguousarray(y.T)


def _need_matmul_skinny(hb, what: str) -> None:
    if not hb.has_packed_matmul_skinny():
        raise MtqError(f"{what} needs {' and '.join(hb.PACKED_MATMUL_SKINNY)}, which this build of libmtq_hip.so lacks: rebuild it from "
                       "this tree")


def matmul(x, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, kernel: str = "block", split: int = 0,
           workspace=None):
    """Y = X·P̂ + b with the packed (k, n) matrix `pt`: (m, k) · (k, n) → (m, n).  For weights stored input-major (y = x @ W) and for
    pack_transposed's result, where it is the linear layer of the (n, k) weight in the transposed layout.  hip (the default when the
    stream is on the device): X an (m, k) bf16 device tensor, bias float32 [n], through mtq_packed_matmul; bit for bit
    linear(kernel="block") on the all-bf16 packing of unpack(pt)ᵀ.  A library without the symbol raises MtqError: no other kernel stands
    in.  emulation: the float64 product of the unpacked matrix, rounded once to float32 (or from there to bf16), as linear's.

    kernel: one of MATMUL_KERNELS.  "block" (the default; any m); "skinny", the split-K kernel for decode (mtq_packed_matmul_skinny,
    m <= 32; `split` slices of K, 0 = the library's choice, and an optional uint8 device `workspace` of
    hip_backend.packed_matmul_skinny_workspace_bytes bytes): bit for bit linear(kernel="skinny") at the same split on the all-bf16
    packing of unpack(pt)ᵀ, and MtqError naming the missing symbols on a library without them; "auto", the skinny kernel for
    m <= AUTO_MATMUL_SKINNY_MAX_M when that is not None and the library has it, else block; from m = AUTO_MATMUL_WIDE_MIN_M on, when
    that is not None and the library has it, the wide-block kernel of matmul_wide, whose bits are the block kernel's.  The skinny and
    the block kernel sum in different orders: each is bit-stable, they may differ in the last bits.  The emulation computes the same
    float64 product under all three names."""
    return _product(_KN, "matmul", x, pt, bias, out_dtype, backend, kernel, split, workspace)


def matmul_wide(x, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None):
    """matmul(kernel="block")'s product and, on hip, its bits, through mtq_packed_matmul_wide: the wide-block kernel for m above the
    decode range (prefill), 128 x 128 outputs to a workgroup, whose waves decode whole tiles of the (k, n) stream.  Correct for any m
    (m = 0 gives (0, n)); faster than the block kernel from m = 64 on, the smallest m measured.  A library without
    the symbol raises MtqError: there is no fall-back to the block kernel here (matmul(kernel="auto") is the call that chooses).
    emulation: matmul's float64 product."""
    return _product_wide(_KN, "matmul_wide", x, pt, bias, out_dtype, backend)


# ----------------------------------------------------------------------------- batches

@dataclass
class PackedBatch:
    """What the tensors of one pack_batch call share.  arena: the uint8 streams back to back (a NumPy array, or a device tensor);
    bases: uint64 [count + 1] on the host, tensor i's stream is arena[64 * bases[i] : 64 * bases[i + 1]]; hip: maps_dev int8
    [count, tiles], offsets_dev int32 [count, tiles + 1] (the uint32 words) and bases_dev int64 [count + 1], the tables the batched
    kernels read.  maps: the host maps, int8 (count, tiles_h, tiles_w): with the arena and the bases they are the whole batch, so the
    grouped linear needs nothing but this object."""

    count: int
    rows: int
    cols: int
    arena: object
    bases: np.ndarray
    maps_dev: object = None
    offsets_dev: object = None
    bases_dev: object = None
    maps: np.ndarray = None


def batch_of(pts):
    """The PackedBatch a list of packed tensors came from, if the list is that batch in order; None otherwise."""
    pts = list(pts)
    if not pts or pts[0]._batch is None:
        return None
    batch = pts[0]._batch[0]
    if len(pts) != batch.count or any(pt._batch is None or pt._batch[0] is not batch or pt._batch[1] != i for i, pt in enumerate(pts)):
        return None
    return batch


def _check_maps(maps, count: int, rows: int, cols: int) -> np.ndarray:
    """Host maps of a batch → int8 (count, tiles_h, tiles_w), every code 0..3."""
    th, tw = -(-rows // TILE), -(-cols // TILE)
    a = np.asarray(maps)
    if a.size != count * th * tw:
        raise MtqError(f"the maps have {a.size} entries, {count} tensors of {th}x{tw} tiles have {count * th * tw}")
    a = np.ascontiguousarray(a.astype(np.int8).reshape(count, th, tw))
    bad = np.flatnonzero(((a < 0) | (a > 3)).reshape(count, -1).any(axis=1))
    if bad.size:
        raise MtqError(f"tensor {int(bad[0])} of the batch: map codes must be MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
    return a


def _batch_shapes(shapes, count: int, rows: int, cols: int) -> list:
    """The original shape of every tensor of the batch: (rows, cols) unless `shapes` names tensors of higher rank with that flatten."""
    if shapes is None:
        return [(rows, cols)] * count
    shapes = [tuple(int(v) for v in s) for s in shapes]
    if len(shapes) != count or any(len(s) < 2 or s[-1] != cols or int(np.prod(s[:-1])) != rows for s in shapes):
        raise MtqError(f"shapes must name {count} tensors whose 2-D flatten is ({rows}, {cols})")
    return shapes


def _pack_batch_device(x3d, maps, rows: int, cols: int, shapes: list, pack_launch) -> list:
    """The hip flow of pack_batch and pack_batch_transposed: `count` packed tensors of rows × cols (th × tw tiles each) from the batch x3d
    through `pack_launch` (hip_backend.pack_tiles_batched, or pack_tiles_transposed_batched for a batch stored cols × rows)."""
    import torch

    count = int(x3d.shape[0])
    th, tw = -(-rows // TILE), -(-cols // TILE)
    tiles = th * tw
    if not _is_torch(x3d):
        x3d = torch.from_numpy(np.ascontiguousarray(x3d, dtype=np.float32))
    if x3d.dtype not in (torch.bfloat16, torch.float32):
        x3d = x3d.to(torch.float32)
    if not x3d.is_cuda:
        x3d = x3d.to(torch.device("cuda", torch.cuda.current_device()))
    if x3d.stride(-1) != 1:
        x3d = x3d.contiguous()
    host_maps = None
    if _is_torch(maps) and maps.is_cuda:
        if maps.dtype != torch.int8 or maps.numel() != count * tiles:
            raise MtqError(f"device maps must be int8 with {count} x {th}x{tw} entries, got {maps.dtype} with {maps.numel()}")
        maps_dev = maps.contiguous().reshape(count, tiles)
    else:
        host_maps = _check_maps(maps.numpy() if _is_torch(maps) else maps, count, rows, cols)
        maps_dev = torch.from_numpy(host_maps.reshape(count, tiles)).to(x3d.device)
    offsets_dev, bases_dev, bad_dev = hb.packed_offsets_device(maps_dev, count, tiles)
    # the one read-back: bases, bad and (device maps) the maps as one byte string
    parts = [bases_dev.view(torch.uint8), bad_dev.view(torch.uint8)] + ([maps_dev.view(torch.uint8).reshape(-1)] if host_maps is None else [])
    back = torch.cat(parts).cpu().numpy()
    bases = back[: 8 * (count + 1)].view(np.uint64).copy()
    bad = back[8 * (count + 1): 8 * (count + 1) + 4 * count].view(np.int32)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise MtqError(f"tensor {i} of the batch: {int(bad[i])} map codes are not MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
    if host_maps is None:
        host_maps = back[8 * (count + 1) + 4 * count:].view(np.int8).reshape(count, th, tw).copy()
    arena = torch.empty((int(bases[count]) * 64,), dtype=torch.uint8, device=x3d.device)
    pack_launch(x3d, maps_dev, offsets_dev, bases_dev, arena)
    batch = PackedBatch(count, rows, cols, arena, bases, maps_dev, offsets_dev, bases_dev, maps=host_maps)
    out = []
    for i in range(count):
        a = host_maps[i]
        offsets = offsets_of(a)
        if int(offsets[-1]) != int(bases[i + 1] - bases[i]):
            raise MtqError(f"tensor {i} of the batch: the device's offsets are not those of the map")
        tables = hb.PackedTables(a, maps_dev[i], offsets_dev[i])
        data = arena[int(bases[i]) * 64: int(bases[i + 1]) * 64]
        out.append(PackedTensor(shapes[i], ("nd", shapes[i]), rows, cols, a, offsets, data, _tables=tables, _batch=(batch, i)))
    return out


def pack_batch(x3d, maps, backend: str = "emulation", layout: str = "rows", shapes=None) -> list:
    """`count` tensors of one 2-D shape and their tile maps → a list of PackedTensor whose streams are slices of one arena.

    x3d: (count, rows, cols), a NumPy array or a torch tensor; on hip a bf16 / float32 device tensor is read in place, whatever its row
    pitch and matrix stride (a [::2] view, a view of a wider buffer).  maps: int8 (count, tiles_h, tiles_w), a NumPy array or (hip) a
    device tensor, e.g. a search's maps that never left the device.  shapes: the tensors' original shapes when they are of higher rank
    than their 2-D flatten.

    hip: host maps are checked on the host and uploaded once; device maps are checked on the device.  The offsets of every map and the
    tensors' bases come from one launch pair, the streams from one more; the call synchronises once, to read back the bases, the count
    of bad codes per tensor and (device maps) the maps.  A tensor with a code outside 0..3 raises MtqError before anything is packed.
    emulation: a loop over the NumPy encoder into one NumPy arena with the same slicing.

    Every returned tensor is a full PackedTensor (unpack, linear, PackedLinear, save); unpack_batch undoes the call in one launch."""
    _check_layout(layout)
    _check_backend(backend)
    if len(x3d.shape) != 3 or 0 in tuple(x3d.shape):
        raise MtqError(f"pack_batch takes a non-empty (count, rows, cols) batch, got {tuple(x3d.shape)}")
    count, rows, cols = (int(v) for v in x3d.shape)
    shapes = _batch_shapes(shapes, count, rows, cols)
    if backend == "hip":
        hb.require_gpu()
        return _pack_batch_device(x3d, maps, rows, cols, shapes, hb.pack_tiles_batched)
    xf = x3d.detach().to("cpu").float().numpy() if _is_torch(x3d) else np.asarray(x3d, dtype=np.float32)
    host_maps = _check_maps(maps.detach().to("cpu").numpy() if _is_torch(maps) else maps, count, rows, cols)
    streams = [encode(xf[i], host_maps[i]) for i in range(count)]
    bases = np.concatenate([[0], np.cumsum([int(o[-1]) for _d, o in streams])]).astype(np.uint64)
    arena = np.concatenate([d for d, _o in streams])
    batch = PackedBatch(count, rows, cols, arena, bases, maps=host_maps)
    return [PackedTensor(shapes[i], ("nd", shapes[i]), rows, cols, host_maps[i], streams[i][1], arena[int(bases[i]) * 64: int(bases[i + 1]) * 64],
                         _batch=(batch, i)) for i in range(count)]


def unpack_batch(pts, backend: str = "emulation", dtype: str = "float32"):
    """The inverse of pack_batch for a list it produced: the (count, rows, cols) reconstructions, float32 (bit for bit K3's) or bfloat16
    (exact).  hip: one launch over the batch's arena → a device tensor (a list that is not one whole batch in order is unpacked tensor by
    tensor, through the same kernels).  emulation: a loop over the NumPy decoder → a NumPy float32 array, or a torch CPU bfloat16 tensor."""
    pts = list(pts)
    if not pts:
        raise MtqError("unpack_batch needs at least one packed tensor")
    for pt in pts:
        _check_layout(pt.layout)
    _check_out_dtype(dtype, "dtype")
    _check_backend(backend)
    rows, cols = pts[0].rows, pts[0].cols
    if any((pt.rows, pt.cols) != (rows, cols) for pt in pts):
        raise MtqError("unpack_batch takes tensors of one 2-D shape")
    import torch

    if backend == "hip":
        hb.require_gpu()
        tdtype = _torch_dtype(dtype)
        batch = batch_of(pts)
        if batch is not None and batch.maps_dev is not None:
            return hb.unpack_tiles_batched(batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, batch.count, rows, cols, tdtype)
        return torch.stack([hb.unpack_tiles(_device_data(pt), pt.tables(), rows, cols, tdtype) for pt in pts])
    bits = np.stack([decode(_host_data(pt), pt.map, pt.offsets, rows, cols) for pt in pts])
    if dtype == "float32":
        return bits.view(np.float32)
    return torch.from_numpy((bits >> np.uint32(16)).astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def _need_batch_transposed(hb, what: str) -> None:
    if not hb.has_packed_batch_transposed():
        raise MtqError(f"{what} needs {' and '.join(hb.PACKED_BATCH_TRANSPOSED)}, which this build of libmtq_hip.so lacks: rebuild it from "
                       "this tree")


def pack_batch_transposed(w3d, maps, backend: str = "emulation") -> list:
    """pack_transposed for a batch: `count` 2-D weights of one shape, w3d (count, n, k), under maps over the TRANSPOSES' tile grid, int8
    (count, ceil(k/32), ceil(n/32)) - what the search pipelines give with layout="transpose" (np.stack([r.assignment ...])), as a NumPy
    array or (hip) a device tensor.  Returns ordinary row-layout PackedTensors of shape (k, n), slices of one arena whose PackedBatch
    has rows = k, cols = n: matmul*, PackedMatmul, unpack and unpack_batch (which give the transposes), as_batch and save_dir take them
    as they are; unpack_batch_transposed gives W's orientation back.

    hip: pack_batch's flow with mtq_pack_tiles_transposed_batched as its pack launch - w3d (a bf16 / float32 device tensor is read in
    place, whatever its row pitch and matrix stride; no transposed copy), one offsets launch pair, one read-back (bases, bad-code
    counts, device maps), one pack launch; a tensor with a code outside 0..3 raises MtqError before anything is packed.  Slice i is byte
    for byte pack_transposed(w3d[i], maps[i]).  emulation: pack_batch of the transposed copies."""
    _check_backend(backend)
    if len(w3d.shape) != 3 or 0 in tuple(w3d.shape):
        raise MtqError(f"pack_batch_transposed takes a non-empty (count, n, k) batch, got {tuple(w3d.shape)}")
    count, n, k = (int(v) for v in w3d.shape)
    th, tw = -(-k // TILE), -(-n // TILE)
    given = tuple(int(v) for v in (maps.shape if _is_torch(maps) else np.shape(maps)))
    if len(given) == 3 and given != (count, th, tw):
        raise MtqError(f"the maps are {'x'.join(map(str, given))}, {count} transposed weights have {count}x{th}x{tw} tiles: "
                       "pack_batch_transposed takes maps over the transposes' grid")
    if backend == "hip":
        _need_batch_transposed(hb, "pack_batch_transposed")
        hb.require_gpu()
        return _pack_batch_device(w3d, maps, k, n, [(k, n)] * count, hb.pack_tiles_transposed_batched)
    wf = w3d.detach().to("cpu").float().numpy() if _is_torch(w3d) else np.asarray(w3d, dtype=np.float32)
    return pack_batch(np.ascontiguousarray(wf.transpose(0, 2, 1)), maps, backend="emulation")


def unpack_batch_transposed(pts, backend: str = "emulation", dtype: str = "float32"):
    """unpack_transposed for a list of equal-shaped packed (k, n) tensors: the (count, n, k) weights whose packed transposes they are,
    float32 (bit for bit K3T's) or bfloat16 (exact).  hip: one launch of mtq_unpack_tiles_transposed_batched when the list is one whole
    batch in order, tensor by tensor through mtq_unpack_tiles_transposed otherwise → a device tensor.  emulation: unpack_batch,
    transposed → a NumPy float32 array, or a torch CPU bfloat16 tensor."""
    pts = list(pts)
    if not pts:
        raise MtqError("unpack_batch_transposed needs at least one packed tensor")
    for pt in pts:
        _check_kn(pt, "unpack_batch_transposed")
    _check_out_dtype(dtype, "dtype")
    _check_backend(backend)
    k, n = pts[0].rows, pts[0].cols
    if any((pt.rows, pt.cols) != (k, n) for pt in pts):
        raise MtqError("unpack_batch_transposed takes tensors of one 2-D shape")
    if backend == "hip":
        import torch

        hb.require_gpu()
        tdtype = _torch_dtype(dtype)
        batch = batch_of(pts)
        if batch is not None and batch.maps_dev is not None:
            _need_batch_transposed(hb, "unpack_batch_transposed")
            return hb.unpack_tiles_transposed_batched(batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev, batch.count, n, k, tdtype)
        _need_matmul(hb, "unpack_batch_transposed")
        return torch.stack([hb.unpack_tiles_transposed(_device_data(pt), pt.tables(), n, k, tdtype) for pt in pts])
    y = unpack_batch(pts, backend="emulation", dtype=dtype)
    return y.transpose(1, 2).contiguous() if _is_torch(y) else np.ascontiguousarray(y.transpose(0, 2, 1))


def _resolve_batch(pts_or_batch) -> PackedBatch:
    """What the grouped entries take → its PackedBatch: a PackedBatch as it is (nothing is walked), a list through as_batch."""
    return pts_or_batch if isinstance(pts_or_batch, PackedBatch) else as_batch(pts_or_batch)


def as_batch(pts, device=None) -> PackedBatch:
    """The PackedBatch of a list of equal-shaped 2-D packed tensors: one arena with tensor i's stream at byte 64 * bases[i], as
    pack_batch lays it out.  A list that already is one whole batch in order is that batch (no copy); any other list, e.g. the tensors
    load_dir returned, is concatenated — once per call, so a caller on a hot path keeps the batch and passes it on (PackedExperts
    does).  hip (the streams are on the device, or `device` is given): the arena and the tables maps_dev / offsets_dev / bases_dev live
    on the device, the offsets computed there and checked against the host's.  emulation: a NumPy arena."""
    pts = list(pts)
    if not pts:
        raise MtqError("as_batch needs at least one packed tensor")
    for pt in pts:
        _check_layout(pt.layout)
        if len(pt.shape) != 2:
            raise MtqError(f"as_batch takes 2-D (n, k) weights, got a packed tensor of shape {pt.shape}")
    rows, cols = pts[0].rows, pts[0].cols
    if any((pt.rows, pt.cols) != (rows, cols) for pt in pts):
        raise MtqError("as_batch takes tensors of one 2-D shape")
    batch = batch_of(pts)
    if batch is not None and (device is None or (_batch_on_device(batch) and batch.arena.device == _torch_device(device))):
        return batch
    count = len(pts)
    bases = np.concatenate([[0], np.cumsum([pt.nbytes // 64 for pt in pts])]).astype(np.uint64)
    maps = np.stack([pt.map for pt in pts]).astype(np.int8)
    if device is None and not any(pt.on_device for pt in pts):
        arena = np.concatenate([_host_data(pt)[: pt.nbytes] for pt in pts])
        return PackedBatch(count, rows, cols, arena, bases, maps=maps)
    import torch

    hb.require_gpu()
    dev = _torch_device(device) if device is not None else next(pt.data.device for pt in pts if pt.on_device)
    parts = [(pt.data if pt.on_device else torch.from_numpy(np.ascontiguousarray(_host_data(pt))))[: pt.nbytes].to(dev) for pt in pts]
    return _device_batch(count, rows, cols, torch.cat(parts), bases, maps)


def _device_batch(count: int, rows: int, cols: int, arena, bases: np.ndarray, maps: np.ndarray) -> PackedBatch:
    """A device arena, its host bases and host maps → the PackedBatch with device tables: the maps uploaded, the offsets and bases
    computed on the device and held to the host's (one read-back)."""
    import torch

    maps_dev = torch.from_numpy(np.ascontiguousarray(maps.reshape(count, -1))).to(arena.device)
    offsets_dev, bases_dev, bad_dev = hb.packed_offsets_device(maps_dev, count, maps_dev.shape[1])
    back = torch.cat([bases_dev.view(torch.uint8), bad_dev.view(torch.uint8)]).cpu().numpy()
    bad = back[8 * (count + 1):].view(np.int32)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise MtqError(f"tensor {i} of the list: {int(bad[i])} map codes are not MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
    if not np.array_equal(back[: 8 * (count + 1)].view(np.uint64), bases):
        raise MtqError("the device's bases are not those of the tensors' offsets")
    return PackedBatch(count, rows, cols, arena, bases, maps_dev, offsets_dev, bases_dev, maps=maps)


def _torch_device(device):
    import torch

    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def _batch_on_device(batch: PackedBatch) -> bool:
    return _is_torch(batch.arena) and bool(batch.arena.is_cuda) and batch.maps_dev is not None


def _host_maps(batch: PackedBatch) -> np.ndarray:
    """int8 (count, tiles_h, tiles_w): the batch's own host maps, or (a batch made by hand) its device maps read back."""
    if batch.maps is not None:
        return np.asarray(batch.maps)
    if batch.maps_dev is None:
        raise MtqError("the batch has no maps: make it with pack_batch or as_batch")
    return batch.maps_dev.cpu().numpy().reshape(batch.count, -(-batch.rows // TILE), -(-batch.cols // TILE))


def batch_to_device(batch: PackedBatch, device="cuda") -> PackedBatch:
    """A host batch (the emulation's) as a device batch: one upload of the arena and the maps; a device batch is returned as it is."""
    if _batch_on_device(batch):
        return batch
    import torch

    hb.require_gpu()
    arena = batch.arena if _is_torch(batch.arena) else torch.from_numpy(np.ascontiguousarray(batch.arena, dtype=np.uint8))
    return _device_batch(batch.count, batch.rows, batch.cols, arena.to(_torch_device(device)), np.asarray(batch.bases, dtype=np.uint64), _host_maps(batch))


def _batch_host_tensors(batch: PackedBatch):
    """(map, offsets, host stream) per tensor of a batch, for the emulation."""
    arena = batch.arena.cpu().numpy() if _is_torch(batch.arena) else np.asarray(batch.arena, dtype=np.uint8)
    maps = _host_maps(batch)
    return [(maps[i], offsets_of(maps[i]), arena[int(batch.bases[i]) * 64: int(batch.bases[i + 1]) * 64]) for i in range(batch.count)]


def _host_group_rows(group_rows, count: int, total_rows: int) -> np.ndarray:
    g = np.asarray(group_rows)
    if g.ndim != 1 or g.size != count + 1:
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got shape {g.shape}")
    if not np.issubdtype(g.dtype, np.integer):
        raise MtqError(f"group_rows must hold integers, got {g.dtype}")
    g = g.astype(np.int64)
    if g[0] != 0 or g[-1] != total_rows:
        raise MtqError(f"group_rows must start at 0 and end at the {total_rows} rows of x, got {int(g[0])} .. {int(g[-1])}")
    if (np.diff(g) < 0).any():
        raise MtqError("group_rows must not decrease")
    return g


def clamp_group_rows(group_rows, total_rows: int):
    """What the kernels make of a device group_rows before any use → (r0, r1), int64 [count] each: r0 = clamp(g[e], 0, T),
    r1 = clamp(g[e + 1], r0, T).  Whatever g holds, 0 <= r0 <= r1 <= T."""
    g = np.asarray(group_rows, dtype=np.int64)
    r0 = np.clip(g[:-1], 0, total_rows)
    return r0, np.minimum(np.maximum(g[1:], r0), total_rows)


GROUPED_KERNELS = ("walk", "chunks", "auto")
# What "auto" means.  The two kernels give the same bits, so this decides time alone, by the rule of DESIGN.md §A.6m: "chunks", because
# in profiles/packed_linear_grouped_chunked.txt its median at split 0 is below the walking entry's minimum on every row, the four rows
# with 4 rows per expert included (0.945–0.952) and the sparse rows at 0.19–0.52.  Shapes and counts outside that record are unmeasured.
GROUPED_AUTO_KERNEL = "chunks"


def _grouped_kernel(o: _Orientation, kernel: str) -> str:
    """`kernel` of the grouped entries, "auto" resolved."""
    _check_kernel(kernel, globals()[o.grouped_kernels])
    return globals()[o.grouped_auto_kernel] if kernel == "auto" else kernel


def _grouped_entry(o: _Orientation, hb, kernel: str, lacks=None):
    """(the launch, its workspace-size function) of hip_backend for a resolved grouped kernel, or "wide" for the wide grouped product.
    A kernel whose predicate says the library lacks it is an error that names its symbols, never another kernel; lacks: (who, hint)
    in place of the orientation's own wording of that error."""
    launch, size, has, who, symbols, hint = o.hb_grouped[kernel]
    if has is not None and not getattr(hb, has)():
        who, hint = lacks or (who, hint)
        names = getattr(hb, symbols, None)           # the name of hip_backend's tuple of the symbols, or the text itself
        raise MtqError(f"{who} needs {symbols if names is None else ' and '.join(names)}, {_LACKS}{hint}")
    return getattr(hb, launch), getattr(hb, size)


def _resolve_group_rows(group_rows, count: int, T: int):
    """→ (group_rows, on_device): a device tensor as it is (the kernel clamps it), anything else checked here, as int64 on the host."""
    on_device = _is_torch(group_rows) and bool(group_rows.is_cuda)
    if not on_device:
        group_rows = _host_group_rows(group_rows.numpy() if _is_torch(group_rows) else group_rows, count, T)
    return group_rows, on_device


def _emulated_group_rows(group_rows, on_device: bool, count: int, T: int):
    """(r0, r1) per group for the emulation: a checked host group_rows as it is, a device one as the kernel clamps it."""
    if not on_device:
        return group_rows[:-1], group_rows[1:]
    if tuple(group_rows.shape) != (count + 1,):      # trusted, as on hip: what the kernel makes of it
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got shape {tuple(group_rows.shape)}")
    return clamp_group_rows(group_rows.cpu().numpy(), T)


def _device_group_rows(group_rows, on_device: bool, device):
    import torch

    return group_rows if on_device else torch.from_numpy(group_rows.astype(np.int32)).to(device)


def _device_bias(bias, device):
    if bias is None or _is_torch(bias):
        return bias
    import torch

    return torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32)).to(device)


def _arena_args(batch: PackedBatch) -> tuple:
    return batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev


def _grouped(o: _Orientation, x, group_rows, pts_or_batch, bias, out_dtype, backend, split, workspace, kernel):
    """linear_grouped and matmul_grouped (kernel "walk" / "chunks", resolved) and the two *_grouped_wide (kernel "wide", no split)."""
    batch = _resolve_batch(pts_or_batch)
    _check_out_dtype(out_dtype)
    backend = backend or ("hip" if _batch_on_device(batch) else "emulation")
    _check_backend(backend)
    count, (n, k) = batch.count, o.n_k(batch)
    if len(x.shape) != 2 or x.shape[1] != k:
        raise MtqError(f"x must be (T, {k}), got {tuple(x.shape)}")
    T = int(x.shape[0])
    group_rows, on_device = _resolve_group_rows(group_rows, count, T)
    if backend == "hip":
        launch, _size = _grouped_entry(o, hb, kernel)            # a missing kernel is refused before any device work
        batch = batch_to_device(batch)
        dtype = _torch_dtype(out_dtype)
        if T == 0:
            import torch

            return torch.zeros((0, n), dtype=dtype, device=batch.arena.device)
        more = {} if kernel == "wide" else {"split": split}
        return launch(x, _device_group_rows(group_rows, on_device, batch.arena.device), *_arena_args(batch), count, n,
                      bias=_device_bias(bias, batch.arena.device), out_dtype=dtype, workspace=workspace, **more)
    xf = _host_f32(x)
    r0, r1 = _emulated_group_rows(group_rows, on_device, count, T)
    b = _host_f64(bias, (count, n), "bias")
    y = np.zeros((T, n), dtype=np.float64)
    for e, (amap, offsets, data) in enumerate(_batch_host_tensors(batch)):
        if r1[e] == r0[e]:
            continue
        w = decode(data, amap, offsets, batch.rows, batch.cols).view(np.float32)
        ye = o.times(xf[r0[e]: r1[e]].astype(np.float64), w.astype(np.float64))
        y[r0[e]: r1[e]] = ye if b is None else ye + b[e][None, :]
    return _round_out(y, out_dtype)


def _grouped_batch(o: _Orientation, x3d, pts_or_batch, bias, out_dtype, backend, split, workspace, kernel):
    """linear_batch and matmul_batch: the grouped product over equal groups of m rows."""
    batch = _resolve_batch(pts_or_batch)
    n, k = o.n_k(batch)
    if len(x3d.shape) != 3 or x3d.shape[0] != batch.count or x3d.shape[2] != k:
        raise MtqError(f"x3d must be ({batch.count}, m, {k}), got {tuple(x3d.shape)}")
    m = int(x3d.shape[1])
    y = globals()[o.grouped](x3d.reshape(batch.count * m, k), m * np.arange(batch.count + 1, dtype=np.int64), batch,
                             bias=bias, out_dtype=out_dtype, backend=backend, split=split, workspace=workspace, kernel=kernel)
    return y.reshape(batch.count, m, n)


def linear_grouped(x, group_rows, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, split: int = 0,
                   workspace=None, kernel: str = "walk"):
    """Y[rows of group e] = X[rows of group e]·Ŵ[e]ᵀ (+ bias[e]) for all experts of a batch at once → (T, n).

    x: (T, k); group_rows: count + 1 entries, group e owning rows [group_rows[e], group_rows[e + 1]) — a list or NumPy array is checked
    here (count + 1 entries, nondecreasing, first 0, last T), a device tensor (int32) is passed on as it is and clamped by the kernel;
    pts_or_batch: a PackedBatch (taken as it is: no per-tensor work before the launch) or a list of equal-shaped 2-D packed tensors,
    which goes through as_batch on every call — all its checks, and for a list that is no pack_batch batch a concatenation; a host
    batch on the hip backend is uploaded on every call (batch_to_device does it once); bias: (count, n) float32 or None.
    hip (the default when the arena is on the device): one launch of mtq_packed_linear_skinny_grouped (two with a split over K; `split`
    and `workspace` as in linear(kernel="skinny")), for decode-sized groups: for every group and 32-row chunk of it the bits of
    linear(kernel="skinny") on that chunk and that expert at the same effective split.  Rows outside every group are zeros.
    kernel (GROUPED_KERNELS): "walk", one wave per (slice, expert, tile row) that walks the expert's 32-row chunks; "chunks",
    mtq_packed_linear_skinny_grouped_chunked, one wave per (slice, chunk, tile row) with the chunk list made on the device, for routings
    with hot experts — the same bits, a workspace at every split, MtqError when the library lacks it; "auto", GROUPED_AUTO_KERNEL.
    emulation: per group the float64 product of the decoded weight, rounded once, as linear does, under every kernel name."""
    return _grouped(_NK, x, group_rows, pts_or_batch, bias, out_dtype, backend, split, workspace, _grouped_kernel(_NK, kernel))


def linear_batch(x3d, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, split: int = 0, workspace=None,
                 kernel: str = "walk"):
    """x3d (count, m, k): expert e multiplies x3d[e] → (count, m, n).  linear_grouped with group_rows = m * arange(count + 1)."""
    return _grouped_batch(_NK, x3d, pts_or_batch, bias, out_dtype, backend, split, workspace, kernel)


def linear_grouped_wide(x, group_rows, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, workspace=None):
    """linear_grouped's product for experts that hold hundreds of rows (MoE prefill), through mtq_packed_linear_wide_grouped: one launch
    in which a workgroup owns 128 rows x 128 columns of one group, so an expert's stream is decoded once per 128 rows, not once per 32 as
    by linear_grouped's kernels.  x, group_rows (host: checked here as by linear_grouped; device int32: passed on as it is and clamped by
    the kernel), pts_or_batch and bias as linear_grouped's; there is no split over K; workspace: an optional uint8 device tensor of
    hip_backend.packed_linear_wide_grouped_workspace_bytes bytes (the block plan: a function of count alone).
    hip: for every group the bits of linear(kernel="block") / linear_wide on the group's rows and that expert - the block family's bits,
    not linear_grouped's: the two families sum in different orders, so the two functions may differ in the last bits, which is why this is
    a function of its own and no GROUPED_KERNELS name.  Rows outside every group are zeros; T = 0 gives (0, n) without a call.  A library
    without the symbol raises MtqError before any device work: no other kernel runs in its place.
    emulation: linear_grouped's float64 product."""
    return _grouped(_NK, x, group_rows, pts_or_batch, bias, out_dtype, backend, 0, workspace, "wide")


# ----------------------------------------------------------------------------- grouped products with (k, n) experts

MATMUL_GROUPED_KERNELS = ("walk", "chunks", "auto")
# What "auto" means for matmul_grouped.  The two kernels give the same bits, so this decides time alone, by the rule of DESIGN.md §A.6m:
# "chunks", because in profiles/packed_matmul_grouped.txt (1) its median at split 0 is below the walking entry's minimum on all four
# skewed rows (0.20-0.54 of it) and (2) on the twelve rows with 1, 4 or 32 rows per expert it is within the run's spread (1.0212) of the
# walking entry's minimum (1.001-1.013).  Shapes, counts and routings outside that record are unmeasured.
MATMUL_GROUPED_AUTO_KERNEL = "chunks"


def matmul_grouped(x, group_rows, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, split: int = 0,
                   workspace=None, kernel: str = "walk"):
    """Y[rows of group e] = X[rows of group e]·P̂[e] (+ bias[e]) for all (k, n) experts of a batch at once → (T, n): linear_grouped for
    experts stored as matmul takes them, batch.rows == k and batch.cols == n.  The batch is a pack_batch_transposed list (the experts of
    a transposed-layout search), as_batch of the entries of a pack_model --store-transposed directory, or pack_batch of input-major
    weights.  x: (T, k); group_rows, pts_or_batch, bias (count, n), split and workspace as linear_grouped's: a host group_rows is
    checked here, a device int32 one is passed on as it is and clamped by the kernel; T = 0 gives (0, n) without a call.
    hip: one launch (two with a split over K) for decode-sized groups: for every group and 32-row chunk of it the bits of
    matmul(kernel="skinny") on that chunk and that expert at the same effective split, hence linear_grouped's on the all-bf16 packings
    of unpack(P̂[e])ᵀ.  Rows outside every group are zeros.  kernel (MATMUL_GROUPED_KERNELS): "walk", mtq_packed_matmul_skinny_grouped,
    one wave per (slice, expert, tile column) that walks the expert's 32-row chunks; "chunks",
    mtq_packed_matmul_skinny_grouped_chunked, one wave per (slice, chunk, tile column) with the chunk list made on the device - the
    same bits, a workspace at every split; "auto", MATMUL_GROUPED_AUTO_KERNEL.  A library without the kernel's symbols raises MtqError
    naming them before any device work: no other kernel runs in its place.
    emulation: per group the float64 product of the decoded (k, n) matrix, rounded once, as matmul does, under every kernel name."""
    return _grouped(_KN, x, group_rows, pts_or_batch, bias, out_dtype, backend, split, workspace, _grouped_kernel(_KN, kernel))


def matmul_batch(x3d, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, split: int = 0, workspace=None,
                 kernel: str = "walk"):
    """x3d (count, m, k): expert e multiplies x3d[e] → (count, m, n).  matmul_grouped with group_rows = m * arange(count + 1)."""
    return _grouped_batch(_KN, x3d, pts_or_batch, bias, out_dtype, backend, split, workspace, kernel)


def matmul_grouped_wide(x, group_rows, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, workspace=None):
    """matmul_grouped's product for experts that hold hundreds of rows (MoE prefill), through mtq_packed_matmul_wide_grouped: one launch
    in which a workgroup owns 128 rows x 128 columns of one group.  Arguments as matmul_grouped's without a split; workspace: an
    optional uint8 device tensor of hip_backend.packed_matmul_wide_grouped_workspace_bytes bytes (the block plan).
    hip: for every group the bits of matmul(kernel="block") / matmul_wide on the group's rows and that expert - the block family's
    bits, not matmul_grouped's, which is why this is a function of its own and no MATMUL_GROUPED_KERNELS name.  Rows outside every group
    are zeros; T = 0 gives (0, n) without a call; a library without the symbol raises MtqError before any device work.
    emulation: matmul_grouped's float64 product."""
    return _grouped(_KN, x, group_rows, pts_or_batch, bias, out_dtype, backend, 0, workspace, "wide")


# ----------------------------------------------------------------------------- the gated product (SwiGLU)

def _check_act(act) -> None:
    if act not in ACTS:
        raise MtqError(f"act must be one of {ACTS}, got {act!r}")


def _glu_host(g64: np.ndarray, u64: np.ndarray, act: str) -> np.ndarray:
    """act(g) * u in float64: the emulation's value before its final rounding."""
    if act == "none":
        return g64 * u64
    with np.errstate(over="ignore", invalid="ignore"):
        return g64 / (1.0 + np.exp(-g64)) * u64


def _need_glu(hb, what: str) -> None:
    if not hb.has_packed_glu():
        raise MtqError(f"{what} needs mtq_glu_combine, mtq_packed_glu_wide and mtq_packed_glu_wide_grouped, which this build of libmtq_hip.so "
                       "lacks: rebuild it from this tree")


def glu(x, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
        backend: Optional[str] = None, kernel: str = "auto"):
    """H = act(X·Ŵgᵀ + bg) * (X·Ŵuᵀ + bu), the first half of a gated MLP, with two packed (n, k) weights of one shape in the row layout.
    act (ACTS): "silu", g / (1 + exp(-g)) * u, or "none", g * u (the bilinear GLU).

    hip (the default when the gate's stream is on the device): X an (m, k) bf16 device tensor, the biases float32 [n] or None.  kernel
    (GLU_KERNELS): "fused", mtq_packed_glu_wide, one launch in which a workgroup holds both projections of its outputs, so X is read
    once and no (m, n) intermediate reaches memory; "unfused", two linear(kernel="block") calls into float32 and hip_backend.glu_combine,
    bit for bit what "fused" gives; "auto": for m <= AUTO_SKINNY_MAX_M two linear(kernel="skinny") calls and the combine (the skinny
    family's sums, which may differ from the block family's in the last bits, as linear(kernel="auto") already does; glu_skinny is the same
    bits from the fused decode kernel), above that "fused" from m = AUTO_GLU_FUSED_MIN_M on when that is not None, "unfused" otherwise.  A
    library without the gated entries raises MtqError under every name: there is no fall-back.
    emulation: float64 throughout from the unpacked weights, g = X·Ŵgᵀ + bg, u likewise, act(g) * u, rounded once to float32 and from
    there to bf16, as linear's emulation rounds; the same value under every kernel name."""
    return _glu(_NK, "glu", x, gate, up, act, bias_gate, bias_up, out_dtype, backend, kernel)


def glu_emulation_f64(xf: np.ndarray, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None) -> np.ndarray:
    """The emulation's float64 (m, n) value before its final rounding: what the accuracy tests measure against."""
    return _glu_f64(_NK, xf, gate, up, act, bias_gate, bias_up)


def _need_glu_skinny(hb, what: str) -> None:
    if not hb.has_packed_glu_skinny():
        raise MtqError(f"{what} needs mtq_packed_glu_skinny and mtq_packed_glu_skinny_grouped, which this build of libmtq_hip.so lacks: "
                       "rebuild it from this tree")


def glu_skinny(x, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
               backend: Optional[str] = None, split: int = 0, workspace=None):
    """glu for decode, m <= SKINNY_MAX_M, from the fused split-K kernel: mtq_packed_glu_skinny, two launches in place of the five of
    glu(kernel="auto") at these m, and at split 0 bit for bit its value; at any `split`, the bits of two linear(kernel="skinny") calls
    into float32 at that split and hip_backend.glu_combine.  `split` and `workspace` as in linear(kernel="skinny"), the workspace of
    hip_backend.packed_glu_skinny_workspace_bytes bytes (never 0), allocated when None.  m > SKINNY_MAX_M and a library without the
    entry raise MtqError: there is no fall-back.
    emulation: glu's float64 value rounded once, whatever m and split."""
    return _glu_skinny(_NK, "glu_skinny", x, gate, up, act, bias_gate, bias_up, out_dtype, backend, split, workspace)


def glu_grouped(x, group_rows, gate_batch, up_batch, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
                backend: Optional[str] = None, kernel: str = "fused", workspace=None):
    """glu for all experts of an MoE layer at once → (T, n): H[rows of group e] = act(X[rows]·Ŵg[e]ᵀ + bg[e]) * (X[rows]·Ŵu[e]ᵀ + bu[e]).
    x, group_rows as linear_grouped_wide's; gate_batch, up_batch: two batches of `count` (n, k) experts each, resolved as
    linear_grouped_wide resolves its argument (a PackedBatch as it is, a list through as_batch); the biases (count, n) float32 or None.
    hip: kernel "fused", mtq_packed_glu_wide_grouped, one launch over both arenas with the block list made on the device (workspace: an
    optional uint8 device tensor of hip_backend.packed_glu_wide_grouped_workspace_bytes bytes); "unfused", two linear_grouped_wide calls
    into float32 and hip_backend.glu_combine over all T rows - the same bits on every row of a group (a row of no group is zero under
    "fused" and act(0) * 0 = 0 under "unfused").  T = 0 gives (0, n) without a call.
    emulation: per group glu's float64 value, rounded once."""
    return _glu_grouped(_NK, x, group_rows, gate_batch, up_batch, act, bias_gate, bias_up, out_dtype, backend, kernel, GLU_GROUPED_KERNELS, 0,
                        workspace)


GLU_SKINNY_GROUPED_KERNELS = ("walk", "chunks", "auto")   # glu_grouped_skinny, glu_matmul_grouped_skinny, moe_glu, moe_down_combine, the modules
# What "auto" means.  The kernels give the same bits, so this decides time alone, by the rule of DESIGN.md §A.6m: "walk", because in
# profiles/packed_glu_skinny_chunked.txt the chunked GLU's median with one row in every expert (64 and 256 experts, both orientations) is
# 1.014–1.021 of the walking entry's minimum, above the run's own spread of 1.013; on the skew rows it is 0.35–0.65.
GLU_SKINNY_GROUPED_AUTO_KERNEL = "walk"


def _glu_skinny_grouped_kernel(kernel: str) -> str:
    """`kernel` of the grouped skinny GLU and the MoE decode stages, "auto" resolved."""
    _check_kernel(kernel, GLU_SKINNY_GROUPED_KERNELS)
    return GLU_SKINNY_GROUPED_AUTO_KERNEL if kernel == "auto" else kernel


def _need_glu_grouped_skinny_chunked(o: _Orientation, hb, what: str) -> None:
    if not hb.glu_grouped_chunked_bound(o.kn):
        raise MtqError(f"{what} needs {' and '.join(hb.PACKED_GLU_SKINNY_GROUPED_CHUNKED[o.kn])}, {_LACKS}")


def glu_grouped_skinny(x, group_rows, gate_batch, up_batch, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
                       backend: Optional[str] = None, split: int = 0, workspace=None, kernel: str = "walk"):
    """glu_grouped for decode-sized groups from the fused split-K kernel: mtq_packed_glu_skinny_grouped, two launches over both arenas.
    The arguments are resolved as glu_grouped resolves them.  Per group the bits of two linear_grouped(kernel="walk") calls into float32
    at that `split` and hip_backend.glu_combine: the skinny family's sums, which may differ from glu_grouped's in the last bits.  Rows
    of no group are zeros.  workspace: an optional uint8 device tensor of hip_backend.packed_glu_skinny_grouped_workspace_bytes bytes.
    T = 0 gives (0, n) without a call; a library without the entry raises MtqError: there is no fall-back.
    kernel (GLU_SKINNY_GROUPED_KERNELS): "walk", one wave per (slice, projection, expert, tile row) that walks the expert's 32-row chunks;
    "chunks", mtq_packed_glu_skinny_grouped_chunked, a wave per 32-row chunk from a plan made on the device, for routings with experts of
    many rows - the same bits for a nondecreasing group_rows, its workspace hip_backend.glu_grouped_chunked_workspace_bytes bytes; "auto", GLU_SKINNY_GROUPED_AUTO_KERNEL.  A library without the kernel asked for raises MtqError, it never runs the other.
    emulation: glu_grouped's value, under every kernel name."""
    return _glu_grouped(_NK, x, group_rows, gate_batch, up_batch, act, bias_gate, bias_up, out_dtype, backend, "skinny", ("skinny",), split,
                        workspace, kernel)


def _glu(o: _Orientation, what: str, x, gate: PackedTensor, up: PackedTensor, act, bias_gate, bias_up, out_dtype, backend, kernel):
    """glu and glu_matmul."""
    _check_pair(o, gate, up, what)
    _check_act(act)
    _check_kernel(kernel, GLU_KERNELS)
    _check_out_dtype(out_dtype)
    backend = backend or ("hip" if gate.on_device else "emulation")
    n, k = o.n_k(gate)
    if backend == "hip":
        import torch

        if x.dim() != 2 or x.shape[1] != k:
            raise MtqError(f"x must be (m, {k}), got {tuple(x.shape)}")
        _needs(o.need_glu, hb, what)
        dtype = _torch_dtype(out_dtype)
        m = int(x.shape[0])
        if kernel == "auto":
            fused_min_m = globals()[o.glu_auto_fused_min_m]
            if _at_most(o, o.glu_auto_skinny_max_m, m):
                kernel = "skinny"
            else:
                kernel = "fused" if fused_min_m is not None and m >= fused_min_m else "unfused"
        if kernel == "fused":
            return getattr(hb, o.hb_glu_fused)(x, _device_data(gate), gate.tables(), _device_data(up), up.tables(), n, act=act, bias_gate=bias_gate,
                                               bias_up=bias_up, out_dtype=dtype)
        if kernel == "skinny":
            _needs(o.need_glu_auto_skinny, hb, f'{what}(kernel="auto")')
        side = getattr(hb, o.hb_skinny if kernel == "skinny" else o.hb_block)
        g = side(x, _device_data(gate), gate.tables(), n, bias=bias_gate, out_dtype=torch.float32)
        u = side(x, _device_data(up), up.tables(), n, bias=bias_up, out_dtype=torch.float32)
        return hb.glu_combine(g, u, act=act, out_dtype=dtype)
    _check_backend(backend)
    xf = _host_f32(x)
    if xf.ndim != 2 or xf.shape[1] != k:
        raise MtqError(f"x must be (m, {k}), got {xf.shape}")
    return _round_out(_glu_f64(o, xf, gate, up, act, bias_gate, bias_up), out_dtype)


def _glu_f64(o: _Orientation, xf, gate: PackedTensor, up: PackedTensor, act, bias_gate, bias_up) -> np.ndarray:
    """glu_emulation_f64 and glu_matmul_emulation_f64."""
    n, _k = o.n_k(gate)
    x64 = np.asarray(xf, dtype=np.float32).astype(np.float64)
    sides = []
    for pt, bias, name in ((gate, bias_gate, "bias_gate"), (up, bias_up, "bias_up")):
        w = decode(_host_data(pt), pt.map, pt.offsets, pt.rows, pt.cols).view(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            y = o.times(x64, w.astype(np.float64))
        b = _host_f64(bias, (n,), name)
        sides.append(y if b is None else y + b[None, :])
    return _glu_host(sides[0], sides[1], act)


def _glu_skinny(o: _Orientation, what: str, x, gate: PackedTensor, up: PackedTensor, act, bias_gate, bias_up, out_dtype, backend, split, workspace):
    """glu_skinny and glu_matmul_skinny."""
    _check_pair(o, gate, up, what)
    _check_act(act)
    _check_out_dtype(out_dtype)
    backend = backend or ("hip" if gate.on_device else "emulation")
    n, k = o.n_k(gate)
    if backend == "hip":
        if x.dim() != 2 or x.shape[1] != k:
            raise MtqError(f"x must be (m, {k}), got {tuple(x.shape)}")
        _needs(o.need_glu_skinny, hb, what)
        if int(x.shape[0]) > SKINNY_MAX_M:
            raise MtqError(f"{what} takes m <= {SKINNY_MAX_M}, got m = {int(x.shape[0])}: {o.glu}(kernel=\"auto\") serves every m")
        return getattr(hb, o.hb_glu_skinny)(x, _device_data(gate), gate.tables(), _device_data(up), up.tables(), n, act=act, bias_gate=bias_gate,
                                            bias_up=bias_up, out_dtype=_torch_dtype(out_dtype), split=split, workspace=workspace)
    return globals()[o.glu](x, gate, up, act=act, bias_gate=bias_gate, bias_up=bias_up, out_dtype=out_dtype, backend=backend)


def _glu_grouped(o: _Orientation, x, group_rows, gate_batch, up_batch, act, bias_gate, bias_up, out_dtype, backend, kernel, kernels, split, workspace,
                 skinny_kernel: str = "walk"):
    """The grouped gated products: `kernel` one of `kernels`, GLU_GROUPED_KERNELS or, from the *_grouped_skinny functions alone,
    ("skinny",), whose frame is skinny_kernel (GLU_SKINNY_GROUPED_KERNELS)."""
    gate_b, up_b = _resolve_batch(gate_batch), _resolve_batch(up_batch)
    _check_act(act)
    _check_kernel(kernel, kernels)
    skinny_kernel = _glu_skinny_grouped_kernel(skinny_kernel)
    _check_out_dtype(out_dtype)
    if (gate_b.count, gate_b.rows, gate_b.cols) != (up_b.count, up_b.rows, up_b.cols):
        raise MtqError(f"the gate and the up batch must hold as many experts of one shape, got {gate_b.count} of {gate_b.rows}x{gate_b.cols} and "
                       f"{up_b.count} of {up_b.rows}x{up_b.cols}")
    backend = backend or ("hip" if _batch_on_device(gate_b) else "emulation")
    _check_backend(backend)
    count, (n, k) = gate_b.count, o.n_k(gate_b)
    if len(x.shape) != 2 or x.shape[1] != k:
        raise MtqError(f"x must be (T, {k}), got {tuple(x.shape)}")
    T = int(x.shape[0])
    group_rows, on_device = _resolve_group_rows(group_rows, count, T)
    if backend == "hip":
        if kernel == "skinny" and skinny_kernel == "chunks":     # a missing kernel is refused before any device work, never replaced
            _need_glu_grouped_skinny_chunked(o, hb, f'{o.glu_grouped_skinny}(kernel="chunks")')
        elif kernel == "skinny":
            _needs(o.need_glu_skinny, hb, o.glu_grouped_skinny)
        else:
            _needs(o.need_glu_grouped, hb, o.glu_grouped)
        gate_b, up_b = batch_to_device(gate_b), batch_to_device(up_b)
        dev = gate_b.arena.device
        dtype = _torch_dtype(out_dtype)
        if T == 0:
            import torch

            return torch.zeros((0, n), dtype=dtype, device=dev)
        group_rows = _device_group_rows(group_rows, on_device, dev)
        bias_gate, bias_up = _device_bias(bias_gate, dev), _device_bias(bias_up, dev)
        if kernel == "skinny":
            more = {"kn": o.kn} if skinny_kernel == "chunks" else {}         # one binding for both orientations
            launch = hb.glu_grouped_chunked if skinny_kernel == "chunks" else getattr(hb, o.hb_glu_grouped_skinny)
            return launch(x, group_rows, _arena_args(gate_b), _arena_args(up_b), count, n, act=act, bias_gate=bias_gate, bias_up=bias_up,
                          out_dtype=dtype, split=split, workspace=workspace, **more)
        if kernel == "fused":
            return getattr(hb, o.hb_glu_grouped_fused)(x, group_rows, _arena_args(gate_b), _arena_args(up_b), count, n, act=act, bias_gate=bias_gate,
                                                       bias_up=bias_up, out_dtype=dtype, workspace=workspace)
        wide = globals()[o.grouped_wide]
        g = wide(x, group_rows, gate_b, bias=bias_gate, out_dtype="float32", backend="hip", workspace=workspace)
        u = wide(x, group_rows, up_b, bias=bias_up, out_dtype="float32", backend="hip", workspace=workspace)
        return hb.glu_combine(g, u, act=act, out_dtype=dtype)
    xf = _host_f32(x)
    r0, r1 = _emulated_group_rows(group_rows, on_device, count, T)
    bg, bu = _host_f64(bias_gate, (count, n), "bias_gate"), _host_f64(bias_up, (count, n), "bias_up")
    h = np.zeros((T, n), dtype=np.float64)
    x64 = xf.astype(np.float64)
    for e, (tg, tu) in enumerate(zip(_batch_host_tensors(gate_b), _batch_host_tensors(up_b))):
        if r1[e] == r0[e]:
            continue
        sides = []
        for (amap, offsets, data), b in ((tg, bg), (tu, bu)):
            w = decode(data, amap, offsets, gate_b.rows, gate_b.cols).view(np.float32)
            y = o.times(x64[r0[e]: r1[e]], w.astype(np.float64))
            sides.append(y if b is None else y + b[e][None, :])
        h[r0[e]: r1[e]] = _glu_host(sides[0], sides[1], act)
    return _round_out(h, out_dtype)


# ----------------------------------------------------------------------------- the gated product over (k, n) weights

def _need_glu_matmul(hb, what: str) -> None:
    if not hb.has_packed_glu() or not hb.has_packed_glu_matmul():
        raise MtqError(f"{what} needs mtq_glu_combine and {' and '.join(hb.PACKED_GLU_MATMUL)}, which this build of libmtq_hip.so lacks: "
                       "rebuild it from this tree")


def _need_glu_matmul_skinny(hb, what: str) -> None:
    if not hb.has_packed_glu_matmul_skinny():
        raise MtqError(f"{what} needs {' and '.join(hb.PACKED_GLU_MATMUL_SKINNY)}, which this build of libmtq_hip.so lacks: rebuild it "
                       "from this tree")


def glu_matmul_emulation_f64(xf: np.ndarray, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None) -> np.ndarray:
    """glu_emulation_f64 for packed (k, n) matrices: g = X·P̂g + bg, u = X·P̂u + bu in float64 on unpack's values, act(g) * u, before the
    final rounding."""
    return _glu_f64(_KN, xf, gate, up, act, bias_gate, bias_up)


def glu_matmul(x, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
               backend: Optional[str] = None, kernel: str = "auto"):
    """H = act(X·P̂g + bg) * (X·P̂u + bu), glu for two packed (k, n) matrices of one shape: what matmul takes - pack_transposed's and
    pack_batch_transposed's results, the entries of a pack_model --store-transposed directory, input-major weights.

    hip (the default when the gate's stream is on the device): X an (m, k) bf16 device tensor, the biases float32 [n] or None.  kernel
    (GLU_KERNELS): "fused", mtq_packed_glu_matmul_wide, one launch in which a workgroup holds both projections of its outputs;
    "unfused", two matmul(kernel="block") calls into float32 and hip_backend.glu_combine, bit for bit what "fused" gives; "auto": for
    m <= AUTO_GLU_MATMUL_SKINNY_MAX_M two matmul(kernel="skinny") calls and the combine (the skinny family's sums; glu_matmul_skinny is
    the same bits from the fused decode kernel), above that "fused" from m = AUTO_GLU_MATMUL_FUSED_MIN_M on when that is not None,
    "unfused" otherwise.  Every route equals glu's of the same name on the all-bf16 row-layout packings of unpack(P̂)ᵀ.  A library without
    the entries raises MtqError under every name: there is no fall-back.
    emulation: float64 throughout from the unpacked matrices (glu_matmul_emulation_f64), rounded once to float32 and from there to
    bf16; the same value under every kernel name."""
    return _glu(_KN, "glu_matmul", x, gate, up, act, bias_gate, bias_up, out_dtype, backend, kernel)


def glu_matmul_skinny(x, gate: PackedTensor, up: PackedTensor, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
                      backend: Optional[str] = None, split: int = 0, workspace=None):
    """glu_matmul for decode, m <= SKINNY_MAX_M, from the fused split-K kernel: mtq_packed_glu_matmul_skinny, two launches in place of
    the five of glu_matmul(kernel="auto") at these m, and at split 0 bit for bit its value; at any `split`, the bits of two
    matmul(kernel="skinny") calls into float32 at that split and hip_backend.glu_combine, hence glu_skinny's on the all-bf16 row-layout
    packings of unpack(P̂)ᵀ.  `split` and `workspace` as in glu_skinny.  m > SKINNY_MAX_M and a library without the entry raise
    MtqError: there is no fall-back.
    emulation: glu_matmul's float64 value rounded once, whatever m and split."""
    return _glu_skinny(_KN, "glu_matmul_skinny", x, gate, up, act, bias_gate, bias_up, out_dtype, backend, split, workspace)


def glu_matmul_grouped(x, group_rows, gate_batch, up_batch, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
                       backend: Optional[str] = None, kernel: str = "fused", workspace=None):
    """glu_matmul for all (k, n) experts of an MoE layer at once → (T, n): glu_grouped for experts stored as matmul_grouped takes them,
    batch.rows == k and batch.cols == n (a pack_batch_transposed list, as_batch of a pack_model --store-transposed directory's entries).
    hip: kernel "fused", mtq_packed_glu_matmul_wide_grouped, one launch over both arenas with the block list made on the device
    (workspace: an optional uint8 device tensor of hip_backend.packed_glu_matmul_wide_grouped_workspace_bytes bytes); "unfused", two
    matmul_grouped_wide calls into float32 and hip_backend.glu_combine over all T rows - the same bits on every row of a group; a row of
    no group is zero under both.  T = 0 gives (0, n) without a call.
    emulation: per group glu_matmul's float64 value, rounded once."""
    return _glu_grouped(_KN, x, group_rows, gate_batch, up_batch, act, bias_gate, bias_up, out_dtype, backend, kernel, GLU_GROUPED_KERNELS, 0,
                        workspace)


def glu_matmul_grouped_skinny(x, group_rows, gate_batch, up_batch, act: str = "silu", bias_gate=None, bias_up=None, out_dtype: str = "float32",
                              backend: Optional[str] = None, split: int = 0, workspace=None, kernel: str = "walk"):
    """glu_matmul_grouped for decode-sized groups from the fused split-K kernel: mtq_packed_glu_matmul_skinny_grouped, two launches over
    both arenas.  Per group the bits of two matmul_grouped(kernel="walk") calls into float32 at that `split` and
    hip_backend.glu_combine: the skinny family's sums, which may differ from glu_matmul_grouped's in the last bits.  Rows of no group are
    zeros.  workspace: an optional uint8 device tensor of hip_backend.packed_glu_matmul_skinny_grouped_workspace_bytes bytes.  T = 0
    gives (0, n) without a call; a library without the entry raises MtqError: there is no fall-back.
    kernel (GLU_SKINNY_GROUPED_KERNELS): as glu_grouped_skinny's; "chunks" is mtq_packed_glu_matmul_skinny_grouped_chunked.
    emulation: glu_matmul_grouped's value, under every kernel name."""
    return _glu_grouped(_KN, x, group_rows, gate_batch, up_batch, act, bias_gate, bias_up, out_dtype, backend, "skinny", ("skinny",), split,
                        workspace, kernel)


# ----------------------------------------------------------------------------- MoE routing: plan, dispatch, combine

MOE_MAX_TOPK = 64           # include/mtq.h MTQ_MOE_MAX_TOPK
MOE_MAX_EXPERTS = 4096       # include/mtq.h MTQ_MOE_MAX_EXPERTS


@dataclass
class MoEPlan:
    """The routing of one MoE forward (include/mtq.h "MoE routing"): slot s = t * topk + j of the router's (tokens, topk) ids.
    group_rows: int32 [count + 1], the exclusive prefix sum of the live slots per expert; row_of: int32 [S], a live slot's row in expert
    order (stable: within an expert rows ascend with s), -1 for a dropped slot; src: int32 [S], the inverse, -1 from row
    R = group_rows[count] on.  Device tensors on hip, NumPy arrays on emulation."""
    group_rows: object
    row_of: object
    src: object
    tokens: int
    topk: int
    count: int

    @property
    def slots(self) -> int:
        return self.tokens * self.topk

    @property
    def on_device(self) -> bool:
        return bool(getattr(self.group_rows, "is_cuda", False))


def _need_moe(hb, what: str) -> None:
    if not hb.has_moe():
        raise MtqError(f"{what} needs mtq_moe_plan, mtq_moe_dispatch and mtq_moe_combine, which this build of libmtq_hip.so lacks: rebuild it "
                       "from this tree")


def _moe_limits(tokens: int, topk: int, count: int) -> None:
    if tokens < 1:
        raise MtqError(f"topk_ids must hold at least one token, got {tokens}")
    if not 1 <= topk <= MOE_MAX_TOPK:
        raise MtqError(f"topk must be 1 .. {MOE_MAX_TOPK}, got {topk}")
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= count <= MOE_MAX_EXPERTS:
        raise MtqError(f"count must be an int in 1 .. {MOE_MAX_EXPERTS}, got {count!r}")
    if tokens * topk >= 2 ** 31:
        raise MtqError(f"tokens * topk must be below 2^31, got {tokens} * {topk}")


def _plan_backend(plan: MoEPlan) -> str:
    return "hip" if plan.on_device else "emulation"


def moe_plan(topk_ids, count: int, backend: Optional[str] = None, workspace=None) -> MoEPlan:
    """The routing plan of a router's expert ids: topk_ids (tokens, topk), int32 or int64 (torch.topk gives int64), → MoEPlan.
    An id outside [0, count) is dropped (expert parallelism passes the ids of another rank's experts that way); a token that names
    one expert twice gets a row for each slot.  1 <= topk <= MOE_MAX_TOPK, 1 <= count <= MOE_MAX_EXPERTS, tokens >= 1.
    hip (the default for a device topk_ids): mtq_moe_plan, a stable counting sort on the device: one launch up to 1024 slots, three
    above; nothing is read back.  workspace: an optional uint8 device tensor of hip_backend.moe_plan_workspace_bytes bytes.
    emulation: NumPy's stable argsort of where(live, id, count); plan.src[:R] is its first R entries."""
    if len(topk_ids.shape) != 2:
        raise MtqError(f"topk_ids must be 2-D (tokens, topk), got shape {tuple(topk_ids.shape)}")
    if str(topk_ids.dtype).replace("torch.", "") not in ("int32", "int64"):
        raise MtqError(f"topk_ids must be int32 or int64, got {topk_ids.dtype}")
    T, K = (int(v) for v in topk_ids.shape)
    _moe_limits(T, K, count)
    count = int(count)
    backend = backend or ("hip" if _is_torch(topk_ids) and topk_ids.is_cuda else "emulation")
    _check_backend(backend)
    if backend == "hip":
        _need_moe(hb, "moe_plan")
        if not _is_torch(topk_ids):
            import torch

            topk_ids = torch.from_numpy(np.ascontiguousarray(topk_ids)).to("cuda")
        group_rows, row_of, src = hb.moe_plan(topk_ids, count, workspace=workspace)
        return MoEPlan(group_rows, row_of, src, T, K, count)
    ids = (topk_ids.detach().to("cpu").numpy() if _is_torch(topk_ids) else np.asarray(topk_ids)).astype(np.int64).reshape(-1)
    live = (ids >= 0) & (ids < count)
    order = np.argsort(np.where(live, ids, count), kind="stable")
    R = int(live.sum())
    src = np.full(T * K, -1, dtype=np.int32)
    src[:R] = order[:R]
    row_of = np.full(T * K, -1, dtype=np.int32)
    row_of[order[:R]] = np.arange(R, dtype=np.int32)
    group_rows = np.concatenate([[0], np.cumsum(np.bincount(ids[live], minlength=count))]).astype(np.int32)
    return MoEPlan(group_rows, row_of, src, T, K, count)


def moe_dispatch(x, plan: MoEPlan, out=None):
    """The tokens' rows in expert order: x (tokens, k) bf16 → xs (S, k), xs[r] = x[plan.src[r] // topk], a bit copy; a row from
    R = group_rows[count] on (and any row whose src is no slot) is all +0.  Every one of the S rows is written, so xs goes to
    linear_grouped / glu_grouped / PackedExpertsMLP with the plan's device group_rows as it is: their rows of no group.  The backend is
    the plan's.  hip: mtq_moe_dispatch, one launch; out: an optional bf16 (S, k) device tensor with contiguous rows.
    emulation: x a CPU tensor or an array, the result of its kind."""
    T, K, S = plan.tokens, plan.topk, plan.slots
    if len(x.shape) != 2 or x.shape[0] != T:
        raise MtqError(f"x must be ({T}, k), got {tuple(x.shape)}")
    if _plan_backend(plan) == "hip":
        _need_moe(hb, "moe_dispatch")
        return hb.moe_dispatch(x, plan.src, K, out=out)
    src = np.asarray(plan.src, dtype=np.int64)
    rows = np.nonzero((src >= 0) & (src < S))[0]
    if _is_torch(x):
        import torch

        xs = torch.zeros((S, x.shape[1]), dtype=x.dtype)
        xs[torch.from_numpy(rows)] = x.detach().to("cpu")[torch.from_numpy(src[rows] // K)]
    else:
        xs = np.zeros((S, x.shape[1]), dtype=np.asarray(x).dtype)
        xs[rows] = np.asarray(x)[src[rows] // K]
    if out is not None:
        out[...] = xs
        return out
    return xs


def moe_combine(ys, topk_weights, plan: MoEPlan, base=None, out_dtype: str = "float32", out=None):
    """The experts' rows back in token order with the router's weights: ys (S, n) bf16 or float32 (rows in expert order; more rows are
    allowed, fewer are not), topk_weights (tokens, topk) float32, base None or (tokens, n) bf16 / float32 (a shared expert's output)
    → y (tokens, n) in out_dtype.  For every token and column a float32 accumulator starts at base (or +0) and takes, for j = 0 ..
    topk - 1 in that order, fl32(acc + fl32(w[t, j] * ys[row_of[t * topk + j]])): product and sum rounded separately, so the result is
    pinned to the bit.  A dropped slot (row outside [0, S)) is skipped, not multiplied by zero: the rows from R on are never read.
    The backend is the plan's.  hip: mtq_moe_combine, one launch; out: an optional (tokens, n) device tensor of out_dtype.
    emulation: the same sequence in NumPy's float32; a bf16 result is rounded to nearest even once."""
    T, K, S = plan.tokens, plan.topk, plan.slots
    _check_out_dtype(out_dtype)
    if tuple(topk_weights.shape) != (T, K):
        raise MtqError(f"topk_weights must be ({T}, {K}), got {tuple(topk_weights.shape)}")
    if str(topk_weights.dtype).replace("torch.", "") != "float32":
        raise MtqError(f"topk_weights must be float32, got {topk_weights.dtype}")
    if len(ys.shape) != 2 or ys.shape[0] < S:
        raise MtqError(f"ys must be ({S}, n), one row per slot, got {tuple(ys.shape)}")
    n = int(ys.shape[1])
    if base is not None and tuple(base.shape) != (T, n):
        raise MtqError(f"base must be ({T}, {n}), got {tuple(base.shape)}")
    if _plan_backend(plan) == "hip":
        import torch

        _need_moe(hb, "moe_combine")
        dev = plan.row_of.device
        if not _is_torch(topk_weights):
            topk_weights = torch.from_numpy(np.ascontiguousarray(topk_weights)).to(dev)
        return hb.moe_combine(ys, plan.row_of, topk_weights, base=base, out_dtype=_torch_dtype(out_dtype),
                              out=out)

    def host32(v):
        return v.detach().to("cpu").float().numpy() if _is_torch(v) else np.asarray(v, dtype=np.float32)

    ys32, w = host32(ys), host32(topk_weights)
    acc = np.zeros((T, n), dtype=np.float32) if base is None else host32(base).copy()
    row_of = np.asarray(plan.row_of, dtype=np.int64).reshape(T, K)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(K):
            r = row_of[:, j]
            t = np.nonzero((r >= 0) & (r < S))[0]
            acc[t] = acc[t] + w[t, j][:, None] * ys32[r[t]]        # float32 throughout: two roundings per term
    y = _round_out(acc, out_dtype)
    if out is not None:
        out[...] = y
        return out
    return y


# ----------------------------------------------------------------------------- MoE decode without the staging copies

MOE_DECODE_ROUTES = ("staged", "fused")      # PackedMoE(decode_route=...)


def _moe_orientation(stored) -> _Orientation:
    if stored not in MOE_STORED:
        raise MtqError(f"stored must be one of {MOE_STORED}, got {stored!r}")
    return _KN if stored == "transpose" else _NK


def _need_moe_decode(hb, what: str, kn: bool, kernel: str = "walk") -> None:
    """The decode stages' symbols for a resolved kernel; "chunks" asks for its own and never for the walking ones."""
    if kernel == "chunks":
        if not hb.moe_decode_chunked_bound(kn):
            names = hb.MOE_GATHER_CHUNKED[kn] + hb.MOE_DOWN_COMBINE_CHUNKED[kn]
            raise MtqError(f"{what} needs {' and '.join(names)}, {_LACKS}")
        return
    if not hb.moe_decode_bound(kn):
        names = hb.MOE_GATHER[kn] + hb.MOE_DOWN_COMBINE[kn]
        raise MtqError(f"{what} needs {' and '.join(names)}, which this build of libmtq_hip.so lacks: rebuild it from this tree")


def _moe_stage_backend(plan: MoEPlan, backend) -> str:
    backend = backend or _plan_backend(plan)
    _check_backend(backend)
    if backend != _plan_backend(plan):
        raise MtqError(f"backend {backend!r} needs a plan made on it: this plan is the {_plan_backend(plan)} backend's")
    return backend


def moe_glu(x, plan: MoEPlan, gate_batch, up_batch, act: str = "silu", out_dtype: str = "bfloat16", stored: str = "rows", split: int = 0,
            workspace=None, backend: Optional[str] = None, kernel: str = "walk"):
    """From the token matrix to the experts' gated rows in one step: x (tokens, k) bf16 → h (S, n) in expert order,
    h[r] = act(x[t]·Ŵg[e]ᵀ) * (x[t]·Ŵu[e]ᵀ) for the slot s = plan.src[r] of token t = s // topk and the expert e that owns row r; rows from
    R = group_rows[count] on are zeros.  stored (MOE_STORED): "rows", the batches hold (n, k) experts; "transpose", (k, n) experts.
    hip: mtq_packed_glu_skinny_grouped_gather (its matmul twin), two launches: the grouped skinny GLU wave reads its X groups from the
    token's own row, so the dispatched (S, k) copy is never written.  Bit for bit moe_dispatch then glu_grouped_skinny
    (glu_matmul_grouped_skinny) at the same `split`.  workspace: an optional uint8 device tensor of
    hip_backend.moe_glu_gather_workspace_bytes bytes.  For decode-sized S: a group above 32 rows is walked in chunks by one wave.
    kernel (GLU_SKINNY_GROUPED_KERNELS): "chunks", mtq_packed_glu_skinny_grouped_chunked_gather (its matmul twin), a wave per 32-row
    chunk and the same bits, for routings with hot experts (the workspace: that size function with kernel="chunks"); "auto",
    GLU_SKINNY_GROUPED_AUTO_KERNEL.  A library without the kernel asked for raises MtqError, it never runs the other.
    emulation: moe_dispatch and the emulated glu_grouped_skinny on the first R rows, composed, under every kernel name."""
    o = _moe_orientation(stored)
    kernel = _glu_skinny_grouped_kernel(kernel)
    gate_b, up_b = _resolve_batch(gate_batch), _resolve_batch(up_batch)
    _check_act(act)
    _check_out_dtype(out_dtype)
    if (gate_b.count, gate_b.rows, gate_b.cols) != (up_b.count, up_b.rows, up_b.cols):
        raise MtqError(f"the gate and the up batch must hold as many experts of one shape, got {gate_b.count} of {gate_b.rows}x{gate_b.cols} and "
                       f"{up_b.count} of {up_b.rows}x{up_b.cols}")
    count, (n, k) = gate_b.count, o.n_k(gate_b)
    T, K, S = plan.tokens, plan.topk, plan.slots
    if count != plan.count:
        raise MtqError(f"the plan is for {plan.count} experts, the batches hold {count}")
    if len(x.shape) != 2 or tuple(x.shape) != (T, k):
        raise MtqError(f"x must be ({T}, {k}), got {tuple(x.shape)}")
    backend = _moe_stage_backend(plan, backend)
    if backend == "hip":
        _need_moe_decode(hb, "moe_glu", o.kn, kernel)            # a missing kernel is refused before any device work
        gate_b, up_b = batch_to_device(gate_b), batch_to_device(up_b)
        return hb.moe_glu_gather(x, plan.src, K, plan.group_rows, _arena_args(gate_b), _arena_args(up_b), count, n, act=act,
                                 out_dtype=_torch_dtype(out_dtype), split=split, workspace=workspace, kn=o.kn, kernel=kernel)
    import torch

    xs = _as_torch(moe_dispatch(x, plan))
    R = int(plan.group_rows[-1])
    h = torch.zeros((S, n), dtype=_torch_dtype(out_dtype))
    if R:
        h[:R] = _as_torch(globals()[o.glu_grouped_skinny](xs[:R], plan.group_rows, gate_b, up_b, act=act, out_dtype=out_dtype, backend="emulation"))
    return h


def moe_down_combine(h, topk_weights, plan: MoEPlan, down_batch, base=None, expert_dtype: str = "float32", out_dtype: str = "float32",
                     stored: str = "rows", split: int = 0, workspace=None, out=None, backend: Optional[str] = None, kernel: str = "walk"):
    """From the experts' gated rows to the layer's output in one step: h (S, n) bf16 in expert order (moe_glu's result), topk_weights
    (tokens, topk) float32, base None or (tokens, k_out) → y (tokens, k_out) in out_dtype: the down projection of every row by its
    expert, rounded as a matrix of expert_dtype would hold it, then moe_combine's weighted sum in its order.
    hip: mtq_packed_linear_skinny_grouped_combine (its matmul twin), two launches: the grouped skinny wave writes float32 partial sums
    and one reduce kernel sums the slices, rounds, weighs and adds, so the experts' (S, k_out) rows are never written.  Bit for bit
    linear_grouped(kernel="walk") (matmul_grouped) into expert_dtype at the same `split`, then moe_combine.  workspace: an optional
    uint8 device tensor of hip_backend.moe_down_combine_workspace_bytes bytes; out: an optional (tokens, k_out) device tensor.
    kernel (GLU_SKINNY_GROUPED_KERNELS): "chunks", mtq_packed_linear_skinny_grouped_chunked_combine (its matmul twin): the plan,
    linear_grouped(kernel="chunks")'s wave and the same reduce, the same bits; "auto", GLU_SKINNY_GROUPED_AUTO_KERNEL.
    emulation: the emulated grouped product on the first R rows and the emulated moe_combine, composed, under every kernel name."""
    o = _moe_orientation(stored)
    kernel = _glu_skinny_grouped_kernel(kernel)
    down = _resolve_batch(down_batch)
    _check_out_dtype(out_dtype)
    _check_out_dtype(expert_dtype, "expert_dtype")
    count, (n, k) = down.count, o.n_k(down)
    T, K, S = plan.tokens, plan.topk, plan.slots
    if count != plan.count:
        raise MtqError(f"the plan is for {plan.count} experts, the batch holds {count}")
    if len(h.shape) != 2 or tuple(h.shape) != (S, k):
        raise MtqError(f"h must be ({S}, {k}), one row per slot, got {tuple(h.shape)}")
    if tuple(topk_weights.shape) != (T, K):
        raise MtqError(f"topk_weights must be ({T}, {K}), got {tuple(topk_weights.shape)}")
    if str(topk_weights.dtype).replace("torch.", "") != "float32":
        raise MtqError(f"topk_weights must be float32, got {topk_weights.dtype}")
    if base is not None and tuple(base.shape) != (T, n):
        raise MtqError(f"base must be ({T}, {n}), got {tuple(base.shape)}")
    backend = _moe_stage_backend(plan, backend)
    if backend == "hip":
        import torch

        _need_moe_decode(hb, "moe_down_combine", o.kn, kernel)
        down = batch_to_device(down)
        if not _is_torch(topk_weights):
            topk_weights = torch.from_numpy(np.ascontiguousarray(topk_weights)).to(plan.row_of.device)
        return hb.moe_down_combine(h, plan.group_rows, *_arena_args(down), count, n, plan.row_of, topk_weights, base=base,
                                   expert_dtype=_torch_dtype(expert_dtype), out_dtype=_torch_dtype(out_dtype), out=out, split=split,
                                   workspace=workspace, kn=o.kn, kernel=kernel)
    import torch

    R = int(plan.group_rows[-1])
    ys = torch.zeros((S, n), dtype=_torch_dtype(expert_dtype))
    if R:
        ys[:R] = _as_torch(globals()[o.grouped](_as_torch(h)[:R], plan.group_rows, down, out_dtype=expert_dtype, backend="emulation", kernel="walk"))
    return moe_combine(ys, topk_weights, plan, base=base, out_dtype=out_dtype, out=out)


# ----------------------------------------------------------------------------- MoE router: scoring and group-limited top-k

MOE_MAX_GROUPS = 64          # include/mtq.h MTQ_MOE_MAX_GROUPS
ROUTE_SCORES = ("softmax", "sigmoid")


@dataclass(frozen=True)
class MoERouting:
    """The parameters of moe_route (include/mtq.h "MoE router"), checked here as far as they can be without the expert count;
    check_count(count) checks the rest.  expects_bias: the model routes with a selection bias (DeepSeek-V3's
    e_score_correction_bias), and PackedMoE.forward_logits refuses a call without one."""
    topk: int
    score: str = "softmax"
    n_group: int = 1
    topk_group: int = 1
    group_top: int = 2
    renormalize: bool = True
    eps: float = 0.0
    scale: float = 1.0
    expects_bias: bool = False

    def __post_init__(self):
        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        if not is_int(self.topk) or not 1 <= self.topk <= MOE_MAX_TOPK:
            raise MtqError(f"topk must be an int in 1 .. {MOE_MAX_TOPK}, got {self.topk!r}")
        if self.score not in ROUTE_SCORES:
            raise MtqError(f"score must be one of {ROUTE_SCORES}, got {self.score!r}")
        if not is_int(self.n_group) or not 1 <= self.n_group <= MOE_MAX_GROUPS:
            raise MtqError(f"n_group must be an int in 1 .. {MOE_MAX_GROUPS}, got {self.n_group!r}")
        if not is_int(self.topk_group) or not 1 <= self.topk_group <= self.n_group:
            raise MtqError(f"topk_group must be an int in 1 .. n_group = {self.n_group}, got {self.topk_group!r}")
        if not is_int(self.group_top) or self.group_top not in (1, 2):
            raise MtqError(f"group_top must be 1 or 2, got {self.group_top!r}")
        if not isinstance(self.renormalize, (bool, np.bool_)):
            raise MtqError(f"renormalize must be a bool, got {self.renormalize!r}")
        for name in ("eps", "scale"):
            v = getattr(self, name)
            with np.errstate(over="ignore"):
                finite = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(np.float32(v)))
            if not finite:
                raise MtqError(f"{name} must be a number that is finite in float32, got {v!r}")

    def check_count(self, count: int) -> None:
        """The limits that need the expert count."""
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= count <= MOE_MAX_EXPERTS:
            raise MtqError(f"count must be an int in 1 .. {MOE_MAX_EXPERTS}, got {count!r}")
        if self.topk > count:
            raise MtqError(f"topk must be at most count = {count}, got {self.topk}")
        if count % self.n_group:
            raise MtqError(f"count = {count} must be a multiple of n_group = {self.n_group}")
        size = count // self.n_group
        if self.topk > self.topk_group * size:
            raise MtqError(f"topk = {self.topk} must be at most topk_group * count / n_group = {self.topk_group * size}")
        if self.group_top > size:
            raise MtqError(f"group_top = {self.group_top} must be at most count / n_group = {size}")


# The routers of public model configurations (config.json of the released checkpoints).
MOE_ROUTINGS: Mapping[str, MoERouting] = MappingProxyType({
    "mixtral": MoERouting(topk=2, score="softmax", renormalize=True),
    "qwen3-moe": MoERouting(topk=8, score="softmax", renormalize=True),
    "deepseek-v2": MoERouting(topk=6, score="softmax", n_group=8, topk_group=3, group_top=1, renormalize=False, scale=16.0),
    "deepseek-v3": MoERouting(topk=8, score="sigmoid", n_group=8, topk_group=4, group_top=2, renormalize=True, eps=1e-20, scale=2.5,
                              expects_bias=True),
})


def _need_moe_route(hb, what: str) -> None:
    if not hb._has(hb.MOE_ROUTE):
        raise MtqError(f"{what} needs mtq_moe_route, which this build of libmtq_hip.so lacks: rebuild it from this tree")


def _route_scores_f32(x: np.ndarray, score: str) -> np.ndarray:
    """The emulation's float32 scores: the row maximum subtracted, NumPy's exp and sum in float32."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if score == "sigmoid":
            return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
        p = np.exp(x - np.fmax.reduce(x, axis=1, keepdims=True))
        return (p / p.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _route_rank_key(key: np.ndarray) -> np.ndarray:
    """A key as the ranking sees it: NaN as -Inf, -0 as +0."""
    return np.where(np.isnan(key), np.float32(-np.inf), key).astype(np.float32) + np.float32(0)


def _route_select(s: np.ndarray, bias, r: MoERouting):
    """The pinned rule of include/mtq.h on float32 scores s (T, count) → (ids int32 (T, topk), weights float32 (T, topk)), whole
    arrays at a time: stable sorts for the ranking, float32 array operations (each rounded once) for the weights."""
    T, count = s.shape
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        k = _route_rank_key(s if bias is None else s + bias[None, :])
        out = np.zeros((T, count), dtype=bool)
        if r.n_group > 1:
            size = count // r.n_group
            top = -np.sort(-k.reshape(T, r.n_group, size), axis=2)[:, :, :2]
            group = _route_rank_key(top[:, :, 0] if r.group_top == 1 else top[:, :, 0] + top[:, :, 1])
            kept = np.argsort(-group, axis=1, kind="stable")[:, :r.topk_group]
            keep = np.zeros((T, r.n_group), dtype=bool)
            np.put_along_axis(keep, kept, True, axis=1)
            out = ~np.repeat(keep, size, axis=1)
        by_key = np.argsort(-k, axis=1, kind="stable")
        order = np.take_along_axis(by_key, np.argsort(np.take_along_axis(out, by_key, axis=1), axis=1, kind="stable"), axis=1)
        ids = order[:, :r.topk].astype(np.int32)
        v = np.take_along_axis(s, ids.astype(np.int64), axis=1)
        scale = np.float32(r.scale)
        if not r.renormalize:
            return ids, (v * scale).astype(np.float32)
        d = v[:, 0].copy()
        for j in range(1, r.topk):
            d = d + v[:, j]
        d = d + np.float32(r.eps)
        return ids, ((v / d[:, None]) * scale).astype(np.float32)


def moe_route(logits, topk: int, score: str = "softmax", bias=None, n_group: int = 1, topk_group: int = 1, group_top: int = 2,
              renormalize: bool = True, eps: float = 0.0, scale: float = 1.0, backend: Optional[str] = None, return_scores: bool = False):
    """The router of an MoE layer behind its GEMM: logits (..., count), bf16 or float32, → (topk_weights float32 (..., topk), topk_ids
    int32 (..., topk)), and the float32 scores (..., count) the selection used when return_scores is set.  The rule is include/mtq.h's
    ("MoE router"), pinned to the bit on the scores: softmax or sigmoid scores; key = score + bias (bias: float32 [count], selection
    only); ranking by key, ties to the lower id, NaN as -Inf; with n_group > 1 the topk_group best groups stay (a group's score its
    best key, group_top = 1, or the sum of its best two, group_top = 2); the topk best remaining experts in rank order; weights
    the scores of the selected experts, with renormalize divided by their sum (added in order, + eps), times scale.
    MOE_ROUTINGS has these parameters for public models, as MoERouting records; PackedMoE(router=...) takes one.
    hip (the default for a device tensor): mtq_moe_route, one launch, nothing read back.  emulation: NumPy, float32 scores and the
    same rule; the result is of the logits' kind (CPU tensors for a tensor, arrays for an array)."""
    r = MoERouting(topk, score, n_group, topk_group, group_top, renormalize, eps, scale)
    if len(logits.shape) < 1 or logits.shape[-1] < 1:
        raise MtqError(f"logits must be (..., count), got shape {tuple(logits.shape)}")
    lead, count = tuple(logits.shape[:-1]), int(logits.shape[-1])
    r.check_count(count)
    dtype = str(logits.dtype).replace("torch.", "")
    if dtype not in ("bfloat16", "float32"):
        raise MtqError(f"logits must be bfloat16 or float32, got {logits.dtype}")
    if bias is not None and tuple(bias.shape) != (count,):
        raise MtqError(f"bias must be ({count},), got {tuple(bias.shape)}")
    T = int(np.prod(lead, dtype=np.int64))
    if T < 1:
        raise MtqError(f"logits must hold at least one token, got shape {tuple(logits.shape)}")
    backend = backend or ("hip" if _is_torch(logits) and logits.is_cuda else "emulation")
    _check_backend(backend)
    if backend == "hip":
        import torch

        _need_moe_route(hb, "moe_route")
        if not _is_torch(logits):
            logits = torch.from_numpy(np.ascontiguousarray(logits)).to("cuda")
        if bias is not None:
            bias = (bias if _is_torch(bias) else torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))).to(
                device=logits.device, dtype=torch.float32).contiguous()
        ids, weights, scores = hb.moe_route(logits.reshape(T, count), r.topk, r.score, bias, r.n_group, r.topk_group, r.group_top,
                                            r.renormalize, r.eps, r.scale, return_scores=return_scores)
        got = (weights.reshape(lead + (r.topk,)), ids.reshape(lead + (r.topk,)))
        return got + (scores.reshape(lead + (count,)),) if return_scores else got
    as_torch = _is_torch(logits)
    x = _host_f32(logits).reshape(T, count)
    b = None if bias is None else _host_f32(bias).reshape(count)
    s = _route_scores_f32(x, r.score)
    ids, weights = _route_select(s, b, r)
    got = (weights.reshape(lead + (r.topk,)), ids.reshape(lead + (r.topk,)))
    if return_scores:
        got += (s.reshape(lead + (count,)),)
    if as_torch:
        import torch

        got = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in got)
    return got


def _named(cls, name: str):
    """A class made by a factory under its public name and its docstring of _CLASS_DOCS."""
    cls.__name__ = cls.__qualname__ = name
    cls.__doc__ = _CLASS_DOCS[name]
    return cls


_CLASS_DOCS = {
    "PackedMLP":
        """A gated MLP over three packed weights, down(act(gate(x)) * up(x)): gate and up (n, k), down (k_out, n).  INFERENCE ONLY, as
        PackedLinear.  forward(x) takes bf16 (..., k), flattens the leading dimensions to m, runs glu(kernel="auto") into bf16 and
        linear(kernel="auto") with `down`, and returns (..., k_out) in out_dtype; m = 0 gives the empty result without a call.
        decode_kernel (MLP_DECODE_KERNELS): "pair", that route at every m; "fused", m <= AUTO_SKINNY_MAX_M goes through glu_skinny
        instead, the same bits from two launches in place of five.""",
    "PackedMatmulMLP":
        """PackedMLP over three packed (k, n) matrices, as matmul takes them: gate and up (k, hidden), down (hidden, k_out) - the
        entries of a pack_model --store-transposed directory, pack_transposed's results, input-major weights.  INFERENCE ONLY.
        forward(x) takes bf16 (..., k), flattens the leading dimensions to m, runs glu_matmul(kernel="auto") into bf16 and
        matmul(kernel="auto") with `down`, and returns (..., k_out) in out_dtype; m = 0 gives the empty result without a call.
        decode_kernel (MATMUL_MLP_DECODE_KERNELS): "pair", that route at every m; "fused", m <= AUTO_GLU_MATMUL_SKINNY_MAX_M goes through
        glu_matmul_skinny instead, the same bits from two launches in place of five.""",
    "PackedExpertsMLP":
        """The gated MLPs of the experts of one MoE layer: three batches of `count` experts, gate and up (n, k), down (k_out, n).
        INFERENCE ONLY.  forward(x, group_rows): x (T, k) bf16, group e owning rows [group_rows[e], group_rows[e + 1]) → (T, k_out):
        glu_grouped (kernel "fused") into bf16, then linear_grouped_wide with the down batch.  The batches are resolved once, here; on hip
        the arenas, their tables and the one plan workspace both launches use stay on the device.  T = 0 gives the empty result.
        decode_max_rows: None, that route at every T; a positive number, a forward with T <= decode_max_rows goes through
        glu_grouped_skinny into bf16 and linear_grouped(kernel="walk") with the down batch instead (the skinny family's sums, which may
        differ from the wide route's in the last bits), with one workspace sized here for decode_max_rows rows.
        decode_grouped_kernel (GLU_SKINNY_GROUPED_KERNELS; not decode_kernel, which is PackedMLP's pair or fused): the kernel of both
        halves of that route.  "walk", the two above; "chunks", glu_grouped_skinny(kernel="chunks") and linear_grouped(kernel="chunks"),
        a wave per 32-row chunk and the same bits, for routings with experts of many rows; "auto", GLU_SKINNY_GROUPED_AUTO_KERNEL.  The
        kept workspace is sized with the chosen kernels' size functions; a name other than "walk" needs decode_max_rows.""",
    "PackedExpertsMatmulMLP":
        """PackedExpertsMLP over three batches of `count` (k, n) experts, as matmul_grouped takes them: gate and up (k, hidden), down
        (hidden, k_out) - pack_batch_transposed lists, or as_batch of a pack_model --store-transposed directory's entries.  INFERENCE
        ONLY.  forward(x, group_rows): x (T, k) bf16 → (T, k_out): glu_matmul_grouped (kernel "fused") into bf16, then
        matmul_grouped_wide with the down batch.  The batches are resolved once, here; on hip the arenas, their tables and the one plan
        workspace both launches use stay on the device.  T = 0 gives the empty result.
        decode_max_rows: None, that route at every T; a positive number, a forward with T <= decode_max_rows goes through
        glu_matmul_grouped_skinny into bf16 and matmul_grouped(kernel="walk") with the down batch instead (the skinny family's sums,
        which may differ from the wide route's in the last bits), with one workspace sized here for decode_max_rows rows.
        decode_grouped_kernel: PackedExpertsMLP's, for glu_matmul_grouped_skinny and matmul_grouped.""",
    "PackedLinear":
        """A linear layer over a packed (n, k) weight.  INFERENCE ONLY: the kernels have no backward, no gradient reaches x, the weight
        or the bias.  forward(x) takes bf16 (..., k), flattens the leading dimensions to m, multiplies through linear() with
        `kernel` ("auto": the skinny split-K kernel for decode-sized m, the block kernel above, the wide-block kernel with the same
        bits from AUTO_WIDE_MIN_M on) and returns (..., n) in out_dtype.
        hip: the tables, the bias and a workspace sized for every m <= 32 stay on the device across calls, so a decode step
        allocates only its output.  emulation: CPU tensors, the float64 product (for use without a GPU).""",
    "PackedMatmul":
        """x @ P̂ + b over a packed (k, n) matrix (pack of an input-major weight, or pack_transposed of an (n, k) one).  INFERENCE ONLY,
        as PackedLinear.  forward(x) takes bf16 (..., k), flattens the leading dimensions to m, multiplies through matmul() and returns
        (..., n) in out_dtype.  hip: the tables and the bias stay on the device across calls; a library without mtq_packed_matmul is
        refused here, not at the first forward.  emulation: CPU tensors, the float64 product.
        kernel: matmul's, "block" by default.  With "skinny" or "auto" on hip one workspace, sized for m = 32 at the library's split,
        stays on the device across calls (its contents never need initialising), so a decode step allocates only its output;
        "skinny" on a library without mtq_packed_matmul_skinny is refused here.""",
    "PackedExperts":
        """The experts of one batch as a module.  INFERENCE ONLY, as PackedLinear.  forward(x, group_rows): x (T, k), group e owning
        rows [group_rows[e], group_rows[e + 1]) → (T, n) through linear_grouped.  The batch is made once, here (as_batch for a list), and
        every forward multiplies with that arena: hip: the arena, its tables and the bias stay on the device, no host work per expert
        and no synchronisation in forward (with a device group_rows), and the workspace grows to the largest T seen.  emulation: CPU tensors, the float64 product.
        kernel: as linear_grouped's, resolved here; the kept workspace is sized by the size function of the kernel in use.
        wide_min_rows: None (the default: every call goes through linear_grouped), or an int: a forward whose x has T >= wide_min_rows
        rows goes through linear_grouped_wide, the wide-block kernel for experts with hundreds of rows (T is known on the host: no
        synchronisation); its plan workspace is allocated once, here, and is the one kept workspace of both routes.  Crossing the threshold changes the summation order (the block
        family's bits above it, the skinny family's below), so the last bits of a row may differ between a call below and a call at or
        above it.  DESIGN.md §A.6n has the measurement that informs the choice of a value.""",
    "PackedExpertsMatmul":
        """PackedExperts for (k, n) experts: the batch is what matmul_grouped takes, in_features = batch.rows, out_features = batch.cols.
        INFERENCE ONLY.  forward(x, group_rows): x (T, k) → (T, n) through matmul_grouped, or, with wide_min_rows set and
        T >= wide_min_rows, through matmul_grouped_wide (the block family's bits above the threshold, the skinny family's below).  The
        batch is made once, here; hip: the arena, its tables, the bias and ONE kept workspace stay on the device (the plan's bytes from
        the start when wide_min_rows is set, grown to the largest need seen).  A library without the symbols of `kernel`, or of the wide
        kernel when wide_min_rows is set, is refused here, not at the first forward.""",
}


def _as_torch(y):
    if _is_torch(y):
        return y
    import torch

    return torch.from_numpy(y)


def _mlp_class(o: _Orientation, name: str):
    """PackedMLP and PackedMatmulMLP."""
    import torch

    def init(self, gate, up, down, act, out_dtype, backend, decode_kernel):
        torch.nn.Module.__init__(self)
        decode_kernels = globals()[o.mlp_decode_kernels]
        if decode_kernel not in decode_kernels:
            raise MtqError(f"decode_kernel must be one of {decode_kernels}, got {decode_kernel!r}")
        _check_pair(o, gate, up, name)
        _check_act(act)
        _check_layout(down.layout)
        n, k = o.n_k(gate)
        if len(down.shape) != 2 or o.n_k(down)[1] != n:
            raise MtqError(f"down must be a 2-D {o.down_shape.format(n=n)} {o.noun}, the packed tensor is {down.shape}")
        _check_out_dtype(out_dtype)
        self.backend = backend or ("hip" if gate.on_device else "emulation")
        _check_backend(self.backend)
        if self.backend == "hip":
            _needs(o.need_glu, hb, name)             # refused here, not at the first forward
            if decode_kernel == "fused":
                _needs(o.need_glu_skinny, hb, f'{name}(decode_kernel="fused")')
            for pt in (gate, up, down):
                _device_data(pt)
                pt.tables()
        self.gate, self.up, self.down, self.act, self.out_dtype, self.decode_kernel = gate, up, down, act, out_dtype, decode_kernel
        self.in_features, self.hidden_features, self.out_features = k, n, o.n_k(down)[0]

    class MLP(torch.nn.Module):
        if o.kn:
            def __init__(self, gate_kn: PackedTensor, up_kn: PackedTensor, down_kn: PackedTensor, act: str = "silu", out_dtype: str = "bfloat16",
                         backend: Optional[str] = None, decode_kernel: str = "pair"):
                init(self, gate_kn, up_kn, down_kn, act, out_dtype, backend, decode_kernel)
        else:
            def __init__(self, gate: PackedTensor, up: PackedTensor, down: PackedTensor, act: str = "silu", out_dtype: str = "bfloat16",
                         backend: Optional[str] = None, decode_kernel: str = "pair"):
                init(self, gate, up, down, act, out_dtype, backend, decode_kernel)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, hidden_features={self.hidden_features}, out_features={self.out_features}, " \
                   f"act={self.act!r}, backend={self.backend!r}"

        @torch.no_grad()
        def forward(self, x):
            if x.shape[-1] != self.in_features:
                raise MtqError(f"x must be (..., {self.in_features}), got {tuple(x.shape)}")
            lead = tuple(x.shape[:-1])
            x2 = x.reshape(-1, self.in_features)
            if x2.shape[0] == 0:
                return torch.zeros(lead + (self.out_features,), dtype=_torch_dtype(self.out_dtype), device=x.device)
            if self.decode_kernel == "fused" and _at_most(o, o.glu_auto_skinny_max_m, x2.shape[0]):
                h = globals()[o.glu_skinny](x2, self.gate, self.up, act=self.act, out_dtype="bfloat16", backend=self.backend)
            else:
                h = globals()[o.glu](x2, self.gate, self.up, act=self.act, out_dtype="bfloat16", backend=self.backend, kernel="auto")
            y = globals()[o.product](h, self.down, out_dtype=self.out_dtype, backend=self.backend, kernel="auto")
            return _as_torch(y).reshape(lead + (self.out_features,))

    return _named(MLP, name)


def _decode_grouped_kernel(decode_grouped_kernel, decode_max_rows) -> str:
    """decode_grouped_kernel of the expert MLPs and PackedMoE, checked and resolved: one kernel for both halves of the decode route."""
    if decode_grouped_kernel not in GLU_SKINNY_GROUPED_KERNELS:
        raise MtqError(f"decode_grouped_kernel must be one of {GLU_SKINNY_GROUPED_KERNELS}, got {decode_grouped_kernel!r}")
    if decode_grouped_kernel != "walk" and decode_max_rows is None:
        raise MtqError(f"decode_grouped_kernel={decode_grouped_kernel!r} needs decode_max_rows: it chooses the kernels of the decode route")
    return _glu_skinny_grouped_kernel(decode_grouped_kernel)


def _experts_mlp_class(o: _Orientation, name: str):
    """PackedExpertsMLP and PackedExpertsMatmulMLP."""
    import torch

    class ExpertsMLP(torch.nn.Module):
        def __init__(self, gate_pts, up_pts, down_pts, act: str = "silu", out_dtype: str = "bfloat16", backend: Optional[str] = None,
                     decode_max_rows: Optional[int] = None, decode_grouped_kernel: str = "walk"):
            super().__init__()
            _check_act(act)
            if decode_max_rows is not None and (isinstance(decode_max_rows, bool) or not isinstance(decode_max_rows, int) or decode_max_rows <= 0):
                raise MtqError(f"decode_max_rows must be None or a positive int, got {decode_max_rows!r}")
            decode_kernel = _decode_grouped_kernel(decode_grouped_kernel, decode_max_rows)
            _check_out_dtype(out_dtype)
            gate, up, down = (_resolve_batch(b) for b in (gate_pts, up_pts, down_pts))
            if (gate.count, gate.rows, gate.cols) != (up.count, up.rows, up.cols):
                raise MtqError("the gate and the up batch must hold as many experts of one shape")
            (n, k), (n_down, k_down) = o.n_k(gate), o.n_k(down)
            if down.count != gate.count or k_down != n:
                raise MtqError(f"the down batch must hold {gate.count} experts of {o.down_shape.format(n=n)}, got {down.count} of {down.rows}x{down.cols}")
            self.backend = backend or ("hip" if _batch_on_device(gate) else "emulation")
            _check_backend(self.backend)
            self._workspace = None
            self._decode_workspace = None
            if self.backend == "hip":
                _needs(o.need_glu_grouped, hb, name)             # refused here, not at the first forward
                if not o.experts_mlp_wide_last:
                    _grouped_entry(o, hb, "wide")
                if decode_max_rows is not None and decode_kernel == "chunks":     # its own symbols, never the walking ones in their place
                    _need_glu_grouped_skinny_chunked(o, hb, f'{name}(decode_grouped_kernel="chunks")')
                    _grouped_entry(o, hb, "chunks")
                elif decode_max_rows is not None:
                    _needs(o.need_glu_skinny, hb, f"{name}(decode_max_rows=...)")
                    _grouped_entry(o, hb, "walk")
                if o.experts_mlp_wide_last and not getattr(hb, o.hb_grouped["wide"][2])():
                    raise MtqError(f"{name} needs {o.hb_grouped['wide'][4]}, which this build of libmtq_hip.so lacks")
                gate, up, down = (batch_to_device(b) for b in (gate, up, down))
                need = getattr(hb, o.hb_glu_grouped_fused_size)(1, gate.count, n, k)   # a function of count alone
                self._workspace = torch.empty((need,), dtype=torch.uint8, device=gate.arena.device)
                if decode_max_rows is not None:      # one buffer for both decode launches: each is done with it before the next starts
                    glu_need = hb.glu_grouped_chunked_workspace_bytes(decode_max_rows, gate.count, n, k, kn=o.kn) if decode_kernel == "chunks" else \
                        getattr(hb, o.hb_glu_grouped_skinny_size)(decode_max_rows, gate.count, n, k)
                    need = max(glu_need,
                               getattr(hb, o.hb_grouped[decode_kernel][1])(decode_max_rows, down.count, n_down, k_down))
                    self._decode_workspace = torch.empty((need,), dtype=torch.uint8, device=gate.arena.device)
            self.decode_max_rows, self.decode_grouped_kernel, self._decode_kernel = decode_max_rows, decode_grouped_kernel, decode_kernel
            self.gate, self.up, self.down, self.act, self.out_dtype = gate, up, down, act, out_dtype
            self.count, self.in_features, self.hidden_features, self.out_features = gate.count, k, n, n_down

        def extra_repr(self) -> str:
            return f"count={self.count}, in_features={self.in_features}, hidden_features={self.hidden_features}, " \
                   f"out_features={self.out_features}, act={self.act!r}, backend={self.backend!r}"

        @torch.no_grad()
        def forward(self, x, group_rows):
            if x.dim() != 2 or x.shape[1] != self.in_features:
                raise MtqError(f"x must be (T, {self.in_features}), got {tuple(x.shape)}")
            if self.decode_max_rows is not None and x.shape[0] <= self.decode_max_rows:
                h = globals()[o.glu_grouped_skinny](x, group_rows, self.gate, self.up, act=self.act, out_dtype="bfloat16", backend=self.backend,
                                                    workspace=self._decode_workspace, kernel=self._decode_kernel)
                return _as_torch(globals()[o.grouped](h, group_rows, self.down, out_dtype=self.out_dtype, backend=self.backend,
                                                      workspace=self._decode_workspace, kernel=self._decode_kernel))
            h = globals()[o.glu_grouped](x, group_rows, self.gate, self.up, act=self.act, out_dtype="bfloat16", backend=self.backend, kernel="fused",
                                         workspace=self._workspace)
            return _as_torch(globals()[o.grouped_wide](h, group_rows, self.down, out_dtype=self.out_dtype, backend=self.backend,
                                                       workspace=self._workspace))

    return _named(ExpertsMLP, name)


MOE_PLAN_TOPK = 8   # PackedMoE sizes its first plan workspace for max_tokens tokens of this many slots each; a larger call regrows it


def _packed_moe_class():
    import torch

    class PackedMoE(torch.nn.Module):
        """One MoE layer on packed experts, from the router's output to the layer's: plan → dispatch → PackedExpertsMLP → combine.
        INFERENCE ONLY.  forward(x, topk_ids, topk_weights, base=None): x (..., k) bf16, topk_ids and topk_weights (..., K) with x's
        leading dimensions (ids int32 or int64, ids outside [0, count) dropped; weights float32), base None or (..., k_out), a shared
        expert's output to start the sums from → (..., k_out) in out_dtype.  The leading dimensions are flattened to T tokens;
        moe_plan, moe_dispatch, the experts on (xs, plan.group_rows) with all S = T * K rows, moe_combine.  T = 0 gives the empty
        result without a call.
        router: None, a MoERouting or a name of MOE_ROUTINGS.  With one, forward_logits(x, router_logits, bias=None, base=None) takes
        the router GEMM's output (..., count), bf16 or float32, runs moe_route with the router's parameters (bias: the float32
        [count] selection bias, required when the routing expects one) and then forward on its ids and weights: on hip one more
        launch and still nothing read back.  The router GEMM itself stays the model's.
        expert_dtype: the type of the experts' rows the combine reads ("float32": the down projection's sums unrounded; "bfloat16":
        half the bytes).  decode_max_rows: PackedExpertsMLP's, compared against S, the rows the experts see.
        stored (MOE_STORED, the word of a pack_model directory's index.json): "rows", the experts are (n, k) batches and run through
        PackedExpertsMLP; "transpose", they are (k, n) batches - gate and up (k, hidden), down (hidden, k_out), what pack_model
        --store-transposed and pack_batch_transposed write - and run through PackedExpertsMatmulMLP.  Plan, dispatch and combine are the same.
        decode_route (MOE_DECODE_ROUTES): "staged", the chain above at every size; "fused" (needs decode_max_rows), a forward with
        S <= decode_max_rows runs plan → moe_glu → moe_down_combine instead: the gather inside the gated product's X loads and the
        combine inside the down projection's reduce, five launches for seven and no (S, k) or (S, k_out) intermediate, bit for bit the
        staged decode route's result; a larger call takes the staged route.  One workspace sized here serves both launches.
        decode_grouped_kernel (GLU_SKINNY_GROUPED_KERNELS): PackedExpertsMLP's, handed to the experts for the staged decode route and
        to moe_glu / moe_down_combine on the fused one, whose workspace is sized for it; "chunks" gives every 32-row chunk of an
        expert a wave of its own, the same bits, for routings with hot experts.  A name other than "walk" needs decode_max_rows, and
        a library without its symbols is refused here.
        hip: no device-to-host copy and no .item() in a forward; the plan workspace is allocated here for max_tokens tokens and
        regrown when a call needs more.  emulation: CPU tensors, for use without a GPU."""

        def __init__(self, gate_pts, up_pts, down_pts, act: str = "silu", out_dtype: str = "bfloat16", expert_dtype: str = "float32",
                     backend: Optional[str] = None, decode_max_rows: Optional[int] = None, max_tokens: int = 4096, stored: str = "rows",
                     router=None, decode_route: str = "staged", decode_grouped_kernel: str = "walk"):
            super().__init__()
            if decode_route not in MOE_DECODE_ROUTES:
                raise MtqError(f"decode_route must be one of {MOE_DECODE_ROUTES}, got {decode_route!r}")
            if decode_route == "fused" and decode_max_rows is None:
                raise MtqError('decode_route="fused" needs decode_max_rows: the fused route is the decode route, for calls of at most that many slots')
            decode_kernel = _decode_grouped_kernel(decode_grouped_kernel, decode_max_rows)
            fused_what = 'PackedMoE(decode_route="fused")' if decode_kernel == "walk" else 'PackedMoE(decode_route="fused", decode_grouped_kernel="chunks")'
            if decode_route == "fused" and backend == "hip" and stored in MOE_STORED:      # before any device work; asked again for a default backend
                _need_moe_decode(hb, fused_what, stored == "transpose", decode_kernel)
            if isinstance(router, str):
                if router not in MOE_ROUTINGS:
                    raise MtqError(f"router must be a MoERouting or one of {tuple(MOE_ROUTINGS)}, got {router!r}")
                router = MOE_ROUTINGS[router]
            if router is not None and not isinstance(router, MoERouting):
                raise MtqError(f"router must be None, a MoERouting or one of {tuple(MOE_ROUTINGS)}, got {router!r}")
            if stored not in MOE_STORED:
                raise MtqError(f"stored must be one of {MOE_STORED}, got {stored!r}")
            _check_out_dtype(out_dtype)
            _check_out_dtype(expert_dtype, "expert_dtype")
            if isinstance(max_tokens, bool) or not isinstance(max_tokens, int) or max_tokens <= 0:
                raise MtqError(f"max_tokens must be a positive int, got {max_tokens!r}")
            experts_name = "PackedExpertsMLP" if stored == "rows" else "PackedExpertsMatmulMLP"
            experts_mlp = globals().get(experts_name) or __getattr__(experts_name)
            self.experts = experts_mlp(gate_pts, up_pts, down_pts, act=act, out_dtype=expert_dtype, backend=backend,
                                       decode_max_rows=decode_max_rows, decode_grouped_kernel=decode_grouped_kernel)
            self.decode_grouped_kernel, self._decode_kernel = decode_grouped_kernel, decode_kernel
            self.backend, self.out_dtype, self.expert_dtype, self.stored = self.experts.backend, out_dtype, expert_dtype, stored
            self.count, self.in_features, self.out_features = self.experts.count, self.experts.in_features, self.experts.out_features
            if self.count > MOE_MAX_EXPERTS:
                raise MtqError(f"PackedMoE takes at most {MOE_MAX_EXPERTS} experts, got {self.count}")
            self.router = router
            if router is not None:
                router.check_count(self.count)
            self._plan_workspace = None
            self.decode_route, self._fused_workspace = decode_route, None
            if self.backend == "hip":
                _need_moe(hb, "PackedMoE")           # refused here, not at the first forward
                if router is not None:
                    _need_moe_route(hb, "PackedMoE(router=...)")
                if decode_route == "fused":          # one buffer for both launches: each is done with it before the next starts
                    kn = stored == "transpose"
                    _need_moe_decode(hb, fused_what, kn, decode_kernel)
                    ex = self.experts
                    need = max(hb.moe_glu_gather_workspace_bytes(decode_max_rows, ex.count, ex.hidden_features, ex.in_features, kn=kn,
                                                                 kernel=decode_kernel),
                               hb.moe_down_combine_workspace_bytes(decode_max_rows, ex.count, ex.out_features, ex.hidden_features, kn=kn,
                                                                   kernel=decode_kernel))
                    self._fused_workspace = torch.empty((need,), dtype=torch.uint8, device=ex.gate.arena.device)
                need = hb.moe_plan_workspace_bytes(max_tokens, MOE_PLAN_TOPK, self.count)
                self._plan_workspace = torch.empty((need,), dtype=torch.uint8, device=self.experts.gate.arena.device)

        def extra_repr(self) -> str:
            return f"count={self.count}, in_features={self.in_features}, out_features={self.out_features}, backend={self.backend!r}"

        @torch.no_grad()
        def forward(self, x, topk_ids, topk_weights, base=None):
            if x.shape[-1] != self.in_features:
                raise MtqError(f"x must be (..., {self.in_features}), got {tuple(x.shape)}")
            lead = tuple(x.shape[:-1])
            if len(topk_ids.shape) != len(lead) + 1 or tuple(topk_ids.shape[:-1]) != lead:
                raise MtqError(f"topk_ids must be {lead + ('K',)}, got {tuple(topk_ids.shape)}")
            K = int(topk_ids.shape[-1])
            if tuple(topk_weights.shape) != lead + (K,):
                raise MtqError(f"topk_weights must be {lead + (K,)}, got {tuple(topk_weights.shape)}")
            if base is not None and tuple(base.shape) != lead + (self.out_features,):
                raise MtqError(f"base must be {lead + (self.out_features,)}, got {tuple(base.shape)}")
            x2 = x.reshape(-1, self.in_features)
            T = int(x2.shape[0])
            if T == 0:
                return torch.zeros(lead + (self.out_features,), dtype=_torch_dtype(self.out_dtype), device=x.device)
            if self.backend == "hip":
                need = hb.moe_plan_workspace_bytes(T, K, self.count)
                if self._plan_workspace.numel() < need:
                    self._plan_workspace = torch.empty((need,), dtype=torch.uint8, device=self._plan_workspace.device)
            plan = moe_plan(topk_ids.reshape(T, K), self.count, backend=self.backend, workspace=self._plan_workspace)
            if self.decode_route == "fused" and plan.slots <= self.experts.decode_max_rows:
                ex = self.experts
                h = moe_glu(x2, plan, ex.gate, ex.up, act=ex.act, out_dtype="bfloat16", stored=self.stored, workspace=self._fused_workspace,
                            backend=self.backend, kernel=self._decode_kernel)
                y = moe_down_combine(h, topk_weights.reshape(T, K), plan, ex.down, base=None if base is None else base.reshape(T, self.out_features),
                                     expert_dtype=self.expert_dtype, out_dtype=self.out_dtype, stored=self.stored,
                                     workspace=self._fused_workspace, backend=self.backend, kernel=self._decode_kernel)
                return _as_torch(y).reshape(lead + (self.out_features,))
            xs = moe_dispatch(x2, plan)
            if self.backend == "hip":
                ys = self.experts(xs, plan.group_rows)               # all S rows: the rows from R on belong to no group and stay zero
            else:                                                    # a host group_rows ends at the rows it is given: the first R
                R = int(plan.group_rows[-1])
                ys = torch.zeros((plan.slots, self.out_features), dtype=_torch_dtype(self.expert_dtype))
                ys[:R] = self.experts(xs[:R], plan.group_rows)
            y = moe_combine(ys, topk_weights.reshape(T, K), plan, base=None if base is None else base.reshape(T, self.out_features),
                            out_dtype=self.out_dtype)
            if not _is_torch(y):
                y = torch.from_numpy(y)
            return y.reshape(lead + (self.out_features,))

        @torch.no_grad()
        def forward_logits(self, x, router_logits, bias=None, base=None):
            """forward on moe_route's ids and weights of router_logits (..., count) under self.router."""
            if self.router is None:
                raise MtqError("forward_logits needs a router: PackedMoE(..., router=MoERouting(...) or a name of MOE_ROUTINGS)")
            lead = tuple(x.shape[:-1])
            if tuple(router_logits.shape) != lead + (self.count,):
                raise MtqError(f"router_logits must be {lead + (self.count,)}, got {tuple(router_logits.shape)}")
            if bias is None and self.router.expects_bias:
                raise MtqError("this routing selects on score + bias: forward_logits needs the model's float32 [count] bias")
            if x.shape[-1] != self.in_features:
                raise MtqError(f"x must be (..., {self.in_features}), got {tuple(x.shape)}")
            if int(np.prod(lead, dtype=np.int64)) == 0:
                return torch.zeros(lead + (self.out_features,), dtype=_torch_dtype(self.out_dtype), device=x.device)
            r = self.router
            weights, ids = moe_route(router_logits, r.topk, r.score, bias, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps,
                                     r.scale, backend=self.backend)
            return self.forward(x, ids, weights, base=base)

    return PackedMoE


def _product_class(o: _Orientation, name: str):
    """PackedLinear and PackedMatmul."""
    import torch

    def init(self, pt, bias, out_dtype, kernel, backend):
        torch.nn.Module.__init__(self)
        _check_rank2(o, pt, name)
        _check_kernel(kernel, globals()[o.kernels])
        _check_out_dtype(out_dtype)
        self.backend = backend or ("hip" if pt.on_device else "emulation")
        _check_backend(self.backend)
        self.packed, self.kernel, self.out_dtype = pt, kernel, out_dtype
        self.out_features, self.in_features = o.n_k(pt)
        self._workspace = None
        if bias is not None and not _is_torch(bias):
            bias = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))
        if self.backend == "hip":
            _needs(o.module_needs, hb, name)
            if kernel == "skinny":
                _needs(o.need_skinny, hb, f'{name}(kernel="skinny")')
            data = _device_data(pt)
            pt.tables()
            if bias is not None:
                bias = bias.detach().to(device=data.device, dtype=torch.float32).contiguous()
            if kernel != "block" and (o.module_size_every_m or getattr(hb, o.has_auto_skinny)()):
                size, (n, k) = getattr(hb, o.hb_skinny_size), o.n_k(pt)
                # every m <= 32, or m = 32 alone (monotone in m: serves every m <= 32)
                need = max(size(m, n, k) for m in (range(1, SKINNY_MAX_M + 1) if o.module_size_every_m else (SKINNY_MAX_M,)))
                self._workspace = torch.empty((need,), dtype=torch.uint8, device=data.device) if need else None
        self.register_buffer("bias", None if bias is None else bias.detach(), persistent=False)

    class Product(torch.nn.Module):
        if o.kn:
            def __init__(self, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, kernel: str = "block"):
                init(self, pt, bias, out_dtype, kernel, backend)
        else:
            def __init__(self, pt: PackedTensor, bias=None, out_dtype: str = "float32", kernel: str = "auto", backend: Optional[str] = None):
                init(self, pt, bias, out_dtype, kernel, backend)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, kernel={self.kernel!r}, " \
                   f"backend={self.backend!r}, packed_bytes={self.packed.nbytes}"

        @torch.no_grad()
        def forward(self, x):
            if x.shape[-1] != self.in_features:
                raise MtqError(f"x must be (..., {self.in_features}), got {tuple(x.shape)}")
            lead = tuple(x.shape[:-1])
            x2 = x.reshape(-1, self.in_features)
            if x2.shape[0] == 0:
                return torch.zeros(lead + (self.out_features,), dtype=_torch_dtype(self.out_dtype), device=x.device)
            y = globals()[o.product](x2, self.packed, bias=self.bias, out_dtype=self.out_dtype, backend=self.backend, kernel=self.kernel,
                                     workspace=self._workspace)
            return _as_torch(y).reshape(lead + (self.out_features,))

    return _named(Product, name)


def _experts_class(o: _Orientation, name: str):
    """PackedExperts and PackedExpertsMatmul."""
    import torch

    class Experts(torch.nn.Module):
        def __init__(self, pts_or_batch, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, split: int = 0,
                     kernel: str = "walk", wide_min_rows: Optional[int] = None):
            super().__init__()
            self.kernel = _grouped_kernel(o, kernel)
            if wide_min_rows is not None and (isinstance(wide_min_rows, bool) or not isinstance(wide_min_rows, (int, np.integer)) or wide_min_rows < 0):
                raise MtqError(f"wide_min_rows must be None or a non-negative int, got {wide_min_rows!r}")
            self.wide_min_rows = None if wide_min_rows is None else int(wide_min_rows)
            _check_out_dtype(out_dtype)
            batch = _resolve_batch(pts_or_batch)                # once: forward hands the batch down and walks no list
            self.backend = backend or ("hip" if _batch_on_device(batch) else "emulation")
            _check_backend(self.backend)
            self._workspace = None
            n, k = o.n_k(batch)
            if self.backend == "hip":
                size = _grouped_entry(o, hb, self.kernel)[1]     # a library without the kernel is refused here, not at the first forward
                if o.experts_keep_size:
                    self._size = size
                wide_size = None if self.wide_min_rows is None else _grouped_entry(o, hb, "wide", o.experts_wide_lacks)[1]
                batch = batch_to_device(batch)
                if wide_size is not None:
                    need = wide_size(1, batch.count, n, k)                                              # a function of count alone
                    self._workspace = torch.empty((need,), dtype=torch.uint8, device=batch.arena.device)   # only ever replaced by a larger one
            self.batch = batch
            self.out_dtype, self.split = out_dtype, int(split)
            self.count, self.in_features, self.out_features = batch.count, k, n
            if bias is not None:
                if not _is_torch(bias):
                    bias = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))
                if tuple(bias.shape) != (self.count, self.out_features):
                    raise MtqError(f"bias must be ({self.count}, {self.out_features}), got {tuple(bias.shape)}")
                bias = bias.detach().to(device=batch.arena.device if self.backend == "hip" else "cpu", dtype=torch.float32).contiguous()
            self.register_buffer("bias", bias, persistent=False)

        def extra_repr(self) -> str:
            return f"count={self.count}, in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, " \
                   f"backend={self.backend!r}, split={self.split}" + ("" if self.kernel == "walk" else f", kernel={self.kernel!r}") + \
                   ("" if self.wide_min_rows is None else f", wide_min_rows={self.wide_min_rows}")

        @torch.no_grad()
        def forward(self, x, group_rows):
            if x.dim() != 2 or x.shape[1] != self.in_features:
                raise MtqError(f"x must be (T, {self.in_features}), got {tuple(x.shape)}")
            T = int(x.shape[0])
            if self.wide_min_rows is not None and T >= self.wide_min_rows:
                return _as_torch(globals()[o.grouped_wide](x, group_rows, self.batch, bias=self.bias, out_dtype=self.out_dtype, backend=self.backend,
                                                           workspace=self._workspace))
            if self.backend == "hip" and T:
                if o.experts_keep_size:
                    size = self._size
                else:                                # looked up at every forward, by name
                    size = _grouped_entry(o, hb, self.kernel)[1]
                need = size(T, self.count, self.out_features, self.in_features, self.split)
                if need and (self._workspace is None or self._workspace.numel() < need):
                    self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.batch.arena.device)
            return _as_torch(globals()[o.grouped](x, group_rows, self.batch, bias=self.bias, out_dtype=self.out_dtype, backend=self.backend,
                                                  split=self.split, workspace=self._workspace, kernel=self.kernel))

    return _named(Experts, name)


def __getattr__(name):
    """PackedLinear, PackedMatmul, PackedExperts, PackedExpertsMatmul, PackedMLP, PackedExpertsMLP, PackedMatmulMLP, PackedExpertsMatmulMLP
    and PackedMoE are torch.nn.Modules: a class is made on first use, so that importing this module does not import torch."""
    makers = {"PackedLinear": (_product_class, _NK), "PackedMatmul": (_product_class, _KN), "PackedExperts": (_experts_class, _NK),
              "PackedExpertsMatmul": (_experts_class, _KN), "PackedMLP": (_mlp_class, _NK), "PackedMatmulMLP": (_mlp_class, _KN),
              "PackedExpertsMLP": (_experts_mlp_class, _NK), "PackedExpertsMatmulMLP": (_experts_mlp_class, _KN), "PackedMoE": (_packed_moe_class,)}
    if name in makers:
        make, *orientation = makers[name]
        cls = make(*orientation, name) if orientation else make()
        globals()[name] = cls
        return cls
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def save(path, pt: PackedTensor) -> None:
    """A plain .npz: format_version, layout, shape, the 2-D flatten's kind, rows, cols, map, offsets, data."""
    kind, v = pt.shape_info
    np.savez(path, format_version=np.int64(FORMAT_VERSION), layout=np.str_(pt.layout), shape=np.asarray(pt.shape, dtype=np.int64),
             flatten_kind=np.str_(kind), rows=np.int64(pt.rows), cols=np.int64(pt.cols), map=pt.map.astype(np.int8),
             offsets=np.asarray(pt.offsets, dtype=np.uint32), data=_host_data(pt)[: pt.nbytes])


def load(path) -> PackedTensor:
    with np.load(path, allow_pickle=False) as z:
        version = int(z["format_version"]) if "format_version" in z.files else None
        if version != FORMAT_VERSION:
            raise MtqError(f"{path}: packed format version {version}, this package reads version {FORMAT_VERSION}")
        layout = str(z["layout"])
        _check_layout(layout)
        shape = tuple(int(v) for v in z["shape"])
        kind, rows, cols = str(z["flatten_kind"]), int(z["rows"]), int(z["cols"])
        amap, offsets, data = z["map"].astype(np.int8), z["offsets"].astype(np.uint32), z["data"].astype(np.uint8)
    info = {"scalar": ("scalar", ()), "vector": ("vector", shape[0] if shape else 0), "nd": ("nd", shape)}[kind]
    amap = _check_map(amap, rows, cols)
    if not np.array_equal(offsets, offsets_of(amap)):
        raise MtqError(f"{path}: the offsets are not those of the map")
    if data.size != int(offsets[-1]) * 64:
        raise MtqError(f"{path}: the stream holds {data.size} bytes, its offsets say {int(offsets[-1]) * 64}")
    return PackedTensor(shape, info, rows, cols, amap, offsets, data, layout=layout)


# ----------------------------------------------------------------------------- a directory of packed tensors

INDEX_NAME = "index.json"


def slug(name: str) -> str:
    """The file-name form of a tensor's name: the one wq uses for a tensor's artifacts (cli._slug, restated here because importing the
    CLI module has side effects on the process environment)."""
    import re

    return re.sub(r"[^a-zA-Z0-9._-]+", "_", name).strip("_") or "tensor"


def save_dir(path, named: dict, meta=None, run=None) -> dict:
    """{tensor name: PackedTensor} → `path`/<slug>.npz through save(), one file per tensor, and `path`/index.json: the format version and,
    per tensor, its file, shape, counts, nbytes and total_bytes, with meta[name] (a dict of JSON values) merged in; run: a dict of JSON
    values about the whole set (what made it), kept under "run".  Two names with one slug get distinct files.  Returns the index."""
    import json
    from pathlib import Path

    root = Path(path)
    root.mkdir(parents=True, exist_ok=True)
    tensors, used = {}, set()
    for name, pt in named.items():
        base = slug(name)
        stem, k = base, 1
        while stem in used:
            stem, k = f"{base}-{k}", k + 1
        used.add(stem)
        save(root / f"{stem}.npz", pt)
        entry = {"file": f"{stem}.npz", "shape": [int(v) for v in pt.shape], "counts": pt.counts(), "nbytes": pt.nbytes, "total_bytes": pt.total_bytes}
        extra = dict((meta or {}).get(name, {}))
        clash = set(extra) & set(entry)
        if clash:
            raise MtqError(f"meta of {name!r} may not set {sorted(clash)}")
        tensors[name] = {**entry, **extra}
    index = {"format_version": FORMAT_VERSION, **({"run": dict(run)} if run else {}), "tensors": tensors}
    (root / INDEX_NAME).write_text(json.dumps(index, indent=1) + "\n", encoding="utf-8")
    return index


def read_index(path) -> dict:
    """The index.json of a directory save_dir wrote, as a dict, after the checks load_dir makes of it (the file is there and its format
    version is this package's): "run" and, per tensor under "tensors", the entry save_dir wrote with the caller's meta - where
    scripts/pack_model.py --store-transposed records "stored": "transpose" and "source_shape" for a tensor whose packed form is its
    transpose's."""
    import json
    from pathlib import Path

    file = Path(path) / INDEX_NAME
    if not file.exists():
        raise MtqError(f"{file} is missing: not a directory of packed tensors")
    index = json.loads(file.read_text(encoding="utf-8"))
    version = index.get("format_version") if isinstance(index, dict) else None
    if version != FORMAT_VERSION:
        raise MtqError(f"{file}: packed format version {version}, this package reads version {FORMAT_VERSION}")
    return index


def load_dir(path, device=None) -> dict:
    """`path` as save_dir wrote it → {tensor name: PackedTensor}, each file checked against its index entry (an unknown format version, a
    missing file, another shape or a stream of another length than the index says is refused).  device: a torch device the streams are
    uploaded to."""
    from pathlib import Path

    root = Path(path)
    file = root / INDEX_NAME
    index = read_index(root)
    out = {}
    for name, entry in index.get("tensors", {}).items():
        f = root / str(entry.get("file"))
        if not f.is_file():
            raise MtqError(f"{f} is missing: {file} lists it for {name!r}")
        pt = load(f)
        if list(pt.shape) != list(entry.get("shape", [])):
            raise MtqError(f"{f}: shape {pt.shape}, the index says {tuple(entry.get('shape', []))}")
        if pt.nbytes != entry.get("nbytes"):
            raise MtqError(f"{f}: the stream holds {pt.nbytes} bytes, the index says {entry.get('nbytes')}")
        if pt.counts() != entry.get("counts"):
            raise MtqError(f"{f}: the map's counts are not the index's")
        if device is not None:
            import torch

            pt.data = torch.from_numpy(pt.data).to(device)
        out[name] = pt
    return out
