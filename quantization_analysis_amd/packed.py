"""Packed mixed-tile weights: the bytes a tile map promises, and a linear layer that multiplies with them.

The format is the one include/mtq.h fixes (row layout; tile t = tr * tiles_w + tc of the zero-padded 2-D flatten; blobs of 2048 / 1088 /
576 / 320 bytes for the map codes 0..3; uint32 offsets in units of 64 bytes).  It is this project's own layout, not TTNN's on-device
tile format.

Two backends:
  "hip"        the C ABI (csrc/mtq_packed.hip) through hip_backend's wrappers; data lives on the device.
  "emulation"  a NumPy encoder and decoder written from the format's description: the byte-level oracle of the GPU tests, and the way
               the feature works without a GPU.

A map over the transposed layout (params["layout"] = "transpose") is refused: a group there runs down a column, and the packed format
holds row groups only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .compression_algorithms.tile_utils import MIXED_TILE_FORMATS, flatten_2d, unflatten_2d
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
        from . import hip_backend as hb

        if self._tables is None:
            self._tables = hb.PackedTables.on_device(self.map, self.offsets, self.data.device if self.on_device else None)
        return self._tables


def _check_layout(layout: str) -> None:
    if layout != "rows":
        raise MtqError(f"the packed format holds the row layout only; a map over layout {layout!r} cannot be packed")


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
    if backend not in BACKENDS:
        raise MtqError(f"backend must be one of {BACKENDS}, got {backend!r}")
    if backend == "hip":
        from . import hip_backend as hb

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
    if dtype not in ("float32", "bfloat16"):
        raise MtqError(f"dtype must be 'float32' or 'bfloat16', got {dtype!r}")
    if backend == "hip":
        import torch

        from . import hip_backend as hb

        hb.require_gpu()
        y = hb.unpack_tiles(_device_data(pt), pt.tables(), pt.rows, pt.cols, torch.float32 if dtype == "float32" else torch.bfloat16)
        return hb.unflatten(y, pt.shape_info)
    if backend != "emulation":
        raise MtqError(f"backend must be one of {BACKENDS}, got {backend!r}")
    bits = decode(_host_data(pt), pt.map, pt.offsets, pt.rows, pt.cols)
    if dtype == "float32":
        y = unflatten_2d(bits.view(np.float32), pt.shape_info)
        return y
    import torch

    half = torch.from_numpy((bits >> np.uint32(16)).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    kind, v = pt.shape_info
    return half.reshape(()) if kind == "scalar" else (half.reshape(-1)[:v] if kind == "vector" else half.reshape(tuple(v)))


def linear(x, pt: PackedTensor, bias=None, out_dtype: str = "float32", backend: Optional[str] = None, kernel: str = "block", split: int = 0,
           workspace=None):
    """Y = X·Ŵᵀ + b with the packed (n, k) weight `pt` (nn.Linear convention).  hip (the default when the stream is on the device):
    X an (m, k) bf16 device tensor, bias float32, through mtq_packed_linear.  emulation: the float64 product of the unpacked weight,
    rounded once to float32 (or from there to bf16) — the reference the GPU tests hold the kernel to, not a fast path.

    kernel: "block" (the default; any m), "skinny" (the split-K kernel for decode, m <= 32; `split` slices of K, 0 = the library's
    choice, and an optional uint8 device `workspace` of hip_backend.packed_linear_skinny_workspace_bytes bytes) or "auto" (skinny for
    m <= AUTO_SKINNY_MAX_M, block above).  The two kernels sum in different orders: each is bit-stable, they may differ in the last
    bits.  The emulation computes the same float64 product under all three names."""
    _check_layout(pt.layout)
    if kernel not in KERNELS:
        raise MtqError(f"kernel must be one of {KERNELS}, got {kernel!r}")
    if len(pt.shape) != 2:
        raise MtqError(f"linear needs a 2-D (n, k) weight, the packed tensor is {pt.shape}")
    backend = backend or ("hip" if pt.on_device else "emulation")
    if out_dtype not in ("float32", "bfloat16"):
        raise MtqError(f"out_dtype must be 'float32' or 'bfloat16', got {out_dtype!r}")
    n, k = pt.rows, pt.cols
    if backend == "hip":
        import torch

        from . import hip_backend as hb

        if x.dim() != 2 or x.shape[1] != k:
            raise MtqError(f"x must be (m, {k}), got {tuple(x.shape)}")
        dtype = torch.float32 if out_dtype == "float32" else torch.bfloat16
        m = int(x.shape[0])
        if kernel == "skinny" and m > SKINNY_MAX_M:
            raise MtqError(f'kernel="skinny" takes m <= {SKINNY_MAX_M}, got m = {m}')
        if kernel == "skinny" or (kernel == "auto" and m <= AUTO_SKINNY_MAX_M):
            return hb.packed_linear_skinny(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=dtype, split=split, workspace=workspace)
        return hb.packed_linear(x, _device_data(pt), pt.tables(), n, bias=bias, out_dtype=dtype)
    if backend != "emulation":
        raise MtqError(f"backend must be one of {BACKENDS}, got {backend!r}")
    import torch

    xf = x.detach().to("cpu").float().numpy() if _is_torch(x) else np.asarray(x, dtype=np.float32)
    if xf.ndim != 2 or xf.shape[1] != k:
        raise MtqError(f"x must be (m, {k}), got {xf.shape}")
    w = decode(_host_data(pt), pt.map, pt.offsets, n, k).view(np.float32)
    y = xf.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        y = y + (bias.detach().to("cpu").double().numpy() if _is_torch(bias) else np.asarray(bias, dtype=np.float64))[None, :]
    with np.errstate(over="ignore"):
        y32 = y.astype(np.float32)
    return y32 if out_dtype == "float32" else torch.from_numpy(y32).to(torch.bfloat16)


def _packed_linear_class():
    import torch

    class PackedLinear(torch.nn.Module):
        """A linear layer over a packed (n, k) weight.  INFERENCE ONLY: the kernels have no backward, no gradient reaches x, the weight
        or the bias.  forward(x) takes bf16 (..., k), flattens the leading dimensions to m, multiplies through linear() with
        `kernel` ("auto": the skinny split-K kernel for decode-sized m, the block kernel above) and returns (..., n) in out_dtype.
        hip: the tables, the bias and a workspace sized for every m <= 32 stay on the device across calls, so a decode step
        allocates only its output.  emulation: CPU tensors, the float64 product (for use without a GPU)."""

        def __init__(self, pt: PackedTensor, bias=None, out_dtype: str = "float32", kernel: str = "auto", backend: Optional[str] = None):
            super().__init__()
            _check_layout(pt.layout)
            if len(pt.shape) != 2:
                raise MtqError(f"PackedLinear needs a 2-D (n, k) weight, the packed tensor is {pt.shape}")
            if kernel not in KERNELS:
                raise MtqError(f"kernel must be one of {KERNELS}, got {kernel!r}")
            if out_dtype not in ("float32", "bfloat16"):
                raise MtqError(f"out_dtype must be 'float32' or 'bfloat16', got {out_dtype!r}")
            self.backend = backend or ("hip" if pt.on_device else "emulation")
            if self.backend not in BACKENDS:
                raise MtqError(f"backend must be one of {BACKENDS}, got {self.backend!r}")
            self.packed, self.kernel, self.out_dtype = pt, kernel, out_dtype
            self.out_features, self.in_features = pt.rows, pt.cols
            self._workspace = None
            if bias is not None and not _is_torch(bias):
                bias = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))
            if self.backend == "hip":
                from . import hip_backend as hb

                data = _device_data(pt)
                pt.tables()
                if bias is not None:
                    bias = bias.detach().to(device=data.device, dtype=torch.float32).contiguous()
                if kernel != "block":
                    need = max(hb.packed_linear_skinny_workspace_bytes(m, pt.rows, pt.cols) for m in range(1, SKINNY_MAX_M + 1))
                    self._workspace = torch.empty((need,), dtype=torch.uint8, device=data.device) if need else None
            self.register_buffer("bias", None if bias is None else bias.detach(), persistent=False)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, kernel={self.kernel!r}, " \
                   f"backend={self.backend!r}, packed_bytes={self.packed.nbytes}"

        @torch.no_grad()
        def forward(self, x):
            if x.shape[-1] != self.in_features:
                raise MtqError(f"x must be (..., {self.in_features}), got {tuple(x.shape)}")
            lead = tuple(x.shape[:-1])
            x2 = x.reshape(-1, self.in_features)
            dtype = torch.float32 if self.out_dtype == "float32" else torch.bfloat16
            if x2.shape[0] == 0:
                return torch.zeros(lead + (self.out_features,), dtype=dtype, device=x.device)
            y = linear(x2, self.packed, bias=self.bias, out_dtype=self.out_dtype, backend=self.backend, kernel=self.kernel,
                       workspace=self._workspace)
            if not _is_torch(y):
                y = torch.from_numpy(y)
            return y.reshape(lead + (self.out_features,))

    return PackedLinear


def __getattr__(name):
    """PackedLinear is a torch.nn.Module: the class is made on first use, so that importing this module does not import torch."""
    if name == "PackedLinear":
        cls = _packed_linear_class()
        globals()["PackedLinear"] = cls
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
