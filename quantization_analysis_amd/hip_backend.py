"""ctypes binding of libmtq_hip.so (include/mtq.h) for PyTorch-ROCm tensors.

This module is the ONLY place the package talks to the GPU.  There is no CPU fallback: if the
shared library is missing, or no HIP device is visible, device entry points raise MtqError.
PyTorch is used for device memory and streams only (tensor.data_ptr(), current stream).
SIGNATURES is the one description of the C ABI; the wrappers below are the only callers of the
library, and each checks what a launch will dereference before it hands a pointer over.
"""
from __future__ import annotations

import ctypes
import functools
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
# MTQ_LIB selects another build of the same library (kernel A/B experiments); default is the in-tree build.
LIB_PATH = Path(os.environ["MTQ_LIB"]).resolve() if os.environ.get("MTQ_LIB") else _PKG / "libmtq_hip.so"

MIXED_TILE_FORMATS = ["bf16", "bfp8", "bfp4", "bfp2"]
FMT_CODE = {"bf16": 0, "bfp8": 1, "bfp4": 2, "bfp2": 3, "fp0": 4}
PROXY_FORMATS = ["mxfp4", "nvfp4"]   # the scalar proxies: mtq_quantize codes 5, 6 and bits 0, 1 of mtq_fp4_proxy_sums' mask
QUANTIZE_CODE = {**FMT_CODE, "mxfp4": 5, "nvfp4": 6}   # mtq_quantize only; the transposed and map entry points take FMT_CODE
METRIC_CODE = {"pcc": 0, "mae": 1, "atol": 2}
DTYPE_BF16, DTYPE_F32 = 0, 1
TILE = 32

MTQ_VERSION = 143   # include/mtq.h MTQ_VERSION: the oldest library this package binds

# Every function include/mtq.h declares: name → (result, parameters, optional).  One letter per C type class: p pointer or array,
# l int64_t, u uint32_t, i int, d double, z size_t, q uint64_t; results also v void, s const char *.  Optional symbols are found by
# name, not by MTQ_VERSION: an older build of the same version (an A/B library at MTQ_LIB) lacks them and still loads.
SIGNATURES = {
    "mtq_version": ("i", "", False),
    "mtq_last_error": ("s", "", False),
    "mtq_device_count": ("i", "p", False),
    "mtq_stats_record_doubles": ("z", "u", False),
    "mtq_shutdown": ("i", "", False),
    "mtq_tile_stats": ("i", "pilllupp", False),
    "mtq_tile_stats_batched": ("i", "pilllllupp", False),
    "mtq_tile_stats_partial": ("i", "pillllluuupp", False),
    "mtq_tile_stats_partial_begin": ("i", "pillllluuupppp", False),
    "mtq_tile_stats_partial_end": ("i", "pillllluppup", False),
    "mtq_tile_stats_listed": ("i", "pillllluuupplppp", False),
    "mtq_quantize": ("i", "pillliplp", False),
    "mtq_apply_assignment": ("i", "pilllpplp", False),
    "mtq_dequant_fp8_block": ("i", "pplllllplp", False),
    "mtq_pack_slim_records": ("i", "plupp", False),
    "mtq_greedy_create": ("i", "ppluiddi", False),
    "mtq_greedy_pass": ("i", "pipl", False),
    "mtq_greedy_assignment": ("i", "pp", False),
    "mtq_greedy_fixed": ("i", "pp", False),
    "mtq_greedy_counts": ("i", "pp", False),
    "mtq_greedy_value": ("i", "pp", False),
    "mtq_greedy_destroy": ("v", "p", False),
    "mtq_tile_scores": ("i", "pluip", False),
    "mtq_threshold_assign": ("i", "plupiiddppplp", False),
    "mtq_columns_from_stats": ("i", "plupdp", False),
    "mtq_columns_from_sums": ("i", "pdp", False),
    "mtq_tile_scores_device": ("i", "pluipp", False),
    "mtq_threshold_assign_device": ("i", "plupiiddppp", False),
    "mtq_columns_scratch_doubles": ("z", "", False),
    "mtq_column_sums_device": ("i", "pluppp", False),
    "mtq_column_sums_device_batched": ("i", "plluppp", False),
    "mtq_rng_create": ("i", "pq", False),
    "mtq_rng_permutation": ("i", "plp", False),
    "mtq_rng_integers": ("i", "pllp", False),
    "mtq_rng_destroy": ("v", "p", False),
    "mtq_greedy_run": ("i", "plupiiddqppp", False),
    "mtq_greedy_run_batch": ("i", "pllupiiddppppi", False),
    "mtq_selftest_slot_ring": ("i", "", False),
    "mtq_device_copy_2d": ("i", "pzpzzzp", False),
    "mtq_knife_tiles_device": ("i", "pilllllppilppp", False),
    "mtq_greedy_scan_scratch_bytes": ("z", "ll", False),
    "mtq_greedy_scan_device": ("i", "pllupiiddpppppzp", False),
    "mtq_greedy_scan_device_ex": ("i", "pllupiiddpppppzpipppp", False),
    "mtq_scan_carry_bytes": ("z", "l", False),
    "mtq_scan_orders_bytes": ("z", "l", False),
    "mtq_scan_orders_device": ("i", "qlipzp", False),
    "mtq_scan_rank_device": ("i", "plipp", True),
    "mtq_tile_stats_partial_begin_early": ("i", "pillllluuuppppup", True),
    "mtq_greedy_scan_device_early": ("i", "pllupiiddpppppzpppppup", True),
    "mtq_debug_scan_ticks": ("i", "p", False),
    "mtq_threshold_enqueue": ("i", "pillllluupiiddppplppppppp", False),
    "mtq_threshold_columns": ("i", "pllupppp", False),
    "mtq_tile_stats_ragged": ("i", "piiupp", False),
    "mtq_knife_tiles_ragged": ("i", "piippilppp", False),
    "mtq_column_sums_device_ragged": ("i", "ppiuppp", False),
    "mtq_threshold_enqueue_ragged": ("i", "piiuupiiddppplppppppp", False),
    "mtq_threshold_columns_ragged": ("i", "ppiupppp", False),
    "mtq_tile_stats_transposed": ("i", "pilllllupp", True),
    "mtq_quantize_transposed": ("i", "pillliplp", True),
    "mtq_apply_assignment_transposed": ("i", "pilllllpplp", True),
    "mtq_knife_tiles_transposed": ("i", "pilllllppilppp", True),
    "mtq_threshold_enqueue_transposed": ("i", "pillllluupiiddppplppppppp", True),
    "mtq_output_error_scratch_doubles": ("z", "ll", True),
    "mtq_output_error": ("i", "plllpillpuppilppzp", True),
    "mtq_fp4_proxy_scratch_doubles": ("z", "lll", True),
    "mtq_fp4_proxy_sums": ("i", "pillllluppzp", True),
    "mtq_output_error_qx": ("i", "plllpillpuppilppzppl", True),
    "mtq_quantize_rows_bf16": ("i", "pllliplp", True),
    "mtq_gram_blocks_scratch_doubles": ("z", "ll", True),
    "mtq_gram_blocks": ("i", "plllpzpzp", True),
    "mtq_tile_error_tables": ("i", "pilllpzppzp", True),
    "mtq_gram_full_scratch_doubles": ("z", "ll", True),
    "mtq_gram_full": ("i", "plllpzpzp", True),
    "mtq_gptq_sweep_scratch_doubles": ("z", "ll", True),
    "mtq_gptq_sweep": ("i", "pilllpzpzplppzp", True),
    "mtq_output_error_transposed": ("i", "plllpillpuppilppzppl", True),
    "mtq_tile_error_tables_transposed": ("i", "pilllpzppzp", True),
    "mtq_tile_sq_error_batched": ("i", "pilllllpp", True),
    "mtq_budget_allocate_scratch_bytes": ("z", "ll", True),
    "mtq_budget_allocate_device": ("i", "plpiupppppzp", True),
    "mtq_debug_k1_grid": ("i", "iliiip", True),
    "mtq_debug_work_counters": ("i", "p", True),
    "mtq_packed_tile_bytes": ("z", "i", True),
    "mtq_packed_offsets": ("i", "plp", True),
    "mtq_pack_tiles": ("i", "pilllpppzp", True),
    "mtq_unpack_tiles": ("i", "pzppllpilp", True),
    "mtq_packed_linear": ("i", "plllpzpplppilp", True),
    "mtq_packed_linear_skinny_workspace_bytes": ("z", "llli", True),
    "mtq_packed_linear_skinny": ("i", "plllpzpplppilipzp", True),
    "mtq_debug_packed_decode": ("i", "ippp", True),
    "mtq_packed_offsets_batched": ("i", "pllpppp", True),
    "mtq_pack_tiles_batched": ("i", "pilllllppppzp", True),
    "mtq_unpack_tiles_batched": ("i", "pzppplllpillp", True),
    "mtq_packed_linear_skinny_grouped_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_linear_skinny_grouped": ("i", "plllppzpppllplpilipzp", True),
    "mtq_packed_linear_wide": ("i", "plllpzpplppilp", True),
    "mtq_packed_linear_skinny_grouped_chunked_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_linear_skinny_grouped_chunked": ("i", "plllppzpppllplpilipzp", True),
    "mtq_packed_linear_wide_grouped_workspace_bytes": ("z", "llll", True),
    "mtq_packed_linear_wide_grouped": ("i", "plllppzpppllplpilpzp", True),
    "mtq_glu_combine": ("i", "plplllipilp", True),
    "mtq_packed_glu_wide": ("i", "plllpzpppzpplppipilp", True),
    "mtq_packed_glu_wide_grouped_workspace_bytes": ("z", "llll", True),
    "mtq_packed_glu_wide_grouped": ("i", "plllppzppppzpppllpplipilpzp", True),
    "mtq_pack_tiles_transposed": ("i", "pilllpppzp", True),
    "mtq_unpack_tiles_transposed": ("i", "pzppllpilp", True),
    "mtq_packed_matmul": ("i", "plllpzpplppilp", True),
    "mtq_packed_matmul_skinny_workspace_bytes": ("z", "llli", True),
    "mtq_packed_matmul_skinny": ("i", "plllpzpplppilipzp", True),
    "mtq_packed_glu_skinny_workspace_bytes": ("z", "llli", True),
    "mtq_packed_glu_skinny": ("i", "plllpzpppzpplppipilipzp", True),
    "mtq_packed_glu_skinny_grouped_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_skinny_grouped": ("i", "plllppzppppzpppllpplipilipzp", True),
    "mtq_packed_matmul_wide": ("i", "plllpzpplppilp", True),
    "mtq_pack_tiles_transposed_batched": ("i", "pilllllppppzp", True),
    "mtq_unpack_tiles_transposed_batched": ("i", "pzppplllpillp", True),
    "mtq_packed_matmul_skinny_grouped_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_matmul_skinny_grouped": ("i", "plllppzpppllplpilipzp", True),
    "mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_matmul_skinny_grouped_chunked": ("i", "plllppzpppllplpilipzp", True),
    "mtq_packed_matmul_wide_grouped_workspace_bytes": ("z", "llll", True),
    "mtq_packed_matmul_wide_grouped": ("i", "plllppzpppllplpilpzp", True),
    "mtq_moe_plan_workspace_bytes": ("z", "lll", True),
    "mtq_moe_plan": ("i", "pillllppppzp", True),
    "mtq_moe_dispatch": ("i", "plllplplp", True),
    "mtq_moe_combine": ("i", "pilpplpillllpilp", True),
    "mtq_moe_route": ("i", "pilllliplliiddplplplp", True),
    "mtq_packed_glu_matmul_wide": ("i", "plllpzpppzpplppipilp", True),
    "mtq_packed_glu_matmul_wide_grouped_workspace_bytes": ("z", "llll", True),
    "mtq_packed_glu_matmul_wide_grouped": ("i", "plllppzppppzpppllpplipilpzp", True),
    "mtq_packed_glu_matmul_skinny_workspace_bytes": ("z", "llli", True),
    "mtq_packed_glu_matmul_skinny": ("i", "plllpzpppzpplppipilipzp", True),
    "mtq_packed_glu_matmul_skinny_grouped_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_matmul_skinny_grouped": ("i", "plllppzppppzpppllpplipilipzp", True),
}
EXPORTS = list(SIGNATURES)   # tests check the library exports exactly these
OPTIONAL_EXPORTS = tuple(name for name, (_r, _p, optional) in SIGNATURES.items() if optional)
# include/mtq_moe_decode.h, which mtq.h includes: the same description of its prototypes, bound by the same _bind; all optional.  A table
# of its own as the header is a file of its own: SIGNATURES and EXPORTS are mtq.h's prototypes, name for name.
MOE_DECODE_SIGNATURES = {
    "mtq_packed_glu_skinny_grouped_gather_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_skinny_grouped_gather": ("i", "pllllpppzppppzpppllpplipilipzp", True),
    "mtq_packed_glu_matmul_skinny_grouped_gather_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_matmul_skinny_grouped_gather": ("i", "pllllpppzppppzpppllpplipilipzp", True),
    "mtq_packed_linear_skinny_grouped_combine_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_linear_skinny_grouped_combine": ("i", "pllppzpppllipplpilllpilipzp", True),
    "mtq_packed_matmul_skinny_grouped_combine_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_matmul_skinny_grouped_combine": ("i", "pllppzpppllipplpilllpilipzp", True),
}
MOE_DECODE_EXPORTS = tuple(MOE_DECODE_SIGNATURES)
# include/mtq_glu_chunked.h, which mtq.h includes after it: the grouped skinny GLU, its gather form and the down projection with the
# combine, each with a wave per 32-row chunk; the walking parent's letters, all optional, a table of its own for the same reason.
GLU_CHUNKED_SIGNATURES = {
    "mtq_packed_glu_skinny_grouped_chunked_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_skinny_grouped_chunked": ("i", "plllppzppppzpppllpplipilipzp", True),
    "mtq_packed_glu_matmul_skinny_grouped_chunked_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_matmul_skinny_grouped_chunked": ("i", "plllppzppppzpppllpplipilipzp", True),
    "mtq_packed_glu_skinny_grouped_chunked_gather_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_skinny_grouped_chunked_gather": ("i", "pllllpppzppppzpppllpplipilipzp", True),
    "mtq_packed_glu_matmul_skinny_grouped_chunked_gather_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_glu_matmul_skinny_grouped_chunked_gather": ("i", "pllllpppzppppzpppllpplipilipzp", True),
    "mtq_packed_linear_skinny_grouped_chunked_combine_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_linear_skinny_grouped_chunked_combine": ("i", "pllppzpppllipplpilllpilipzp", True),
    "mtq_packed_matmul_skinny_grouped_chunked_combine_workspace_bytes": ("z", "lllli", True),
    "mtq_packed_matmul_skinny_grouped_chunked_combine": ("i", "pllppzpppllipplpilllpilipzp", True),
}
GLU_CHUNKED_EXPORTS = tuple(GLU_CHUNKED_SIGNATURES)
_CTYPE = {"p": ctypes.c_void_p, "l": ctypes.c_int64, "u": ctypes.c_uint32, "i": ctypes.c_int, "d": ctypes.c_double, "z": ctypes.c_size_t,
          "q": ctypes.c_uint64, "v": None, "s": ctypes.c_char_p}


class MtqError(RuntimeError):
    pass


_lib = None
_REBUILD = f"rebuild it from this tree (`make -C {_PKG / 'csrc'}`)"


def build(force: bool = False) -> Path:
    """Compile libmtq_hip.so for gfx950 with hipcc (csrc/Makefile).  Cross-compiles without a GPU."""
    import subprocess

    srcs = list((_PKG / "csrc").glob("*")) + list((_PKG.parent / "include").glob("*.h"))
    stale = not LIB_PATH.exists() or any(p.stat().st_mtime > LIB_PATH.stat().st_mtime for p in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", str(_PKG / "csrc"), "-s"])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise MtqError(
            f"{LIB_PATH} is missing: build it with `make -C {_PKG / 'csrc'}` (hipcc --offload-arch=gfx950). "
            "The hip backend has no CPU fallback."
        )
    # PyTorch-ROCm bundles its own libamdhip64; it must be the ONE HIP runtime of the process, so torch is
    # imported before libmtq_hip.so resolves its libamdhip64.so dependency (two runtimes → "no usable device").
    import torch  # noqa: F401

    L = ctypes.CDLL(str(LIB_PATH))
    _bind(L)
    _lib = L
    # torch registered its exit hooks when it was imported above; a hook registered now runs BEFORE them: the library's threads,
    # events and device tables are released while the HIP runtime is still there (mtq_shutdown; nothing is left to static destructors)
    import atexit

    atexit.register(shutdown)
    return L


def _bind(L) -> None:
    """Sets every symbol's result and parameter types from SIGNATURES, the version first: an older library fails with its version,
    not with the first symbol it lacks."""
    version = getattr(L, "mtq_version", None)
    if version is None:
        raise MtqError(f"{LIB_PATH} has no mtq_version: {_REBUILD}")
    version.restype, version.argtypes = ctypes.c_int, []
    found = version()
    if found < MTQ_VERSION:
        raise MtqError(f"{LIB_PATH} is version {found}, older than this package (it needs {MTQ_VERSION}): {_REBUILD}")
    for name, (result, params, optional) in (*SIGNATURES.items(), *MOE_DECODE_SIGNATURES.items(), *GLU_CHUNKED_SIGNATURES.items()):
        fn = getattr(L, name, None)
        if fn is None:
            if optional:
                continue
            raise MtqError(f"{LIB_PATH} has no {name}: {_REBUILD}")
        fn.restype, fn.argtypes = _CTYPE[result], [_CTYPE[c] for c in params]


def shutdown() -> None:
    """mtq_shutdown: joins the scan threads, drains the devices the library used and frees its device tables and events.  Idempotent;
    registered with atexit by lib().  The library sets itself up again if it is used afterwards."""
    if _lib is not None:
        _lib.mtq_shutdown()


def check(rc: int) -> None:
    if rc != 0:
        raise MtqError(f"libmtq_hip error {rc}: {lib().mtq_last_error().decode()}")


def fmt_mask(formats) -> int:
    m = 0
    for f in formats:
        m |= 1 << MIXED_TILE_FORMATS.index(f)
    return m


def mask_formats(mask: int) -> list[str]:
    return [f for i, f in enumerate(MIXED_TILE_FORMATS) if mask & (1 << i)]


MASK_BF16_IDENTITY = 0x10  # include/mtq.h MTQ_MASK_BF16_IDENTITY (host functions only)
MASK_SLIM = 0x20           # include/mtq.h MTQ_MASK_SLIM (pcc greedy scan on 3-double slots)


def parse_cpulist(text: str) -> set:
    """'0-63,128-191' (sysfs cpulist) → set of CPU numbers."""
    cpus = set()
    for part in text.strip().split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def bind_to_gpu_numa_node(device_index: int) -> str:
    """Restrict this process (and the threads it creates later: scan pool, pinned-memory allocation) to the CPUs of the NUMA
    node its GPU hangs off, read from sysfs through the device's PCI address.  The records are DMA-written into pinned host
    memory and then read by the scan threads: on a two-socket host both want that memory on the GPU's socket.  Returns a
    short description; does nothing (and says so) when the topology cannot be read.  MTQ_NUMA_BIND=0 disables it."""
    from .settings import settings

    if not settings().numa_bind or not hasattr(os, "sched_setaffinity"):
        return "off"
    try:
        p = _torch().cuda.get_device_properties(device_index)
        bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        with open(f"/sys/bus/pci/devices/{bdf}/numa_node") as f:
            node = int(f.read())
        if node < 0:
            return f"{bdf}: no NUMA node reported"
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            allowed = parse_cpulist(f.read()) & os.sched_getaffinity(0)
        if not allowed:
            return f"{bdf}: node {node} has no allowed CPU"
        os.sched_setaffinity(0, allowed)
        return f"{bdf} -> NUMA node {node} ({len(allowed)} CPUs)"
    except (OSError, ValueError, AttributeError, RuntimeError) as exc:
        return f"unavailable ({type(exc).__name__})"


def record_doubles(mask: int) -> int:
    return 2 + (3 if mask & MASK_SLIM else 5) * bin(mask & 0xF).count("1")


def pack_slim_records(stats_dev, mask: int, out=None):
    """Device copy of K1's records [..., tiles, 2+5F] without Σ|d| and max: [..., tiles, 2+3F] (mtq_pack_slim_records)."""
    torch = _torch()
    require_gpu()
    lead = tuple(stats_dev.shape[:-1])
    T = int(np.prod(lead))
    if out is None:
        out = torch.empty(lead + (record_doubles(mask | MASK_SLIM),), dtype=torch.float64, device=stats_dev.device)
    check(lib().mtq_pack_slim_records(stats_dev.data_ptr(), T, mask & 0xF, out.data_ptr(), _stream_ptr()))
    return out


def tiles_hw(rows: int, cols: int) -> tuple[int, int]:
    return -(-rows // TILE), -(-cols // TILE)


# ----------------------------------------------------------------------------- device helpers

def _torch():
    import torch

    return torch


def require_gpu() -> None:
    torch = _torch()
    if not torch.cuda.is_available():
        raise MtqError("backend 'hip' needs a visible MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
    n = ctypes.c_int(0)
    check(lib().mtq_device_count(ctypes.byref(n)))


def _dtype_code(t) -> int:
    torch = _torch()
    if t.dtype == torch.bfloat16:
        return DTYPE_BF16
    if t.dtype == torch.float32:
        return DTYPE_F32
    raise MtqError(f"hip backend takes bfloat16 or float32 tensors, got {t.dtype}")


def _stream_ptr() -> int:
    return _torch().cuda.current_stream().cuda_stream


def _matrix(x, ranks=(2, 3)):
    """The checks before a matrix pointer is taken, in the order rank, contiguous rows, storage type, device (the first three need no
    device) → (storage code, count, stride_elems, rows, cols, ld) of a (rows, cols) or (count, rows, cols) tensor; a 2-D tensor is a
    batch of one.  ld and stride_elems of a single row or matrix are what the kernels' bounds and alignment checks expect."""
    if x.dim() not in ranks:
        raise MtqError(f"expected a {' or '.join(f'{d}-D' for d in ranks)} device tensor, got {x.dim()}-D")
    if x.stride(-1) != 1:
        raise MtqError("expected a device tensor with contiguous rows (stride(-1) == 1)")
    code = _dtype_code(x)
    if not x.is_cuda:
        raise MtqError("expected a device tensor (the hip backend has no CPU fallback)")
    count, rows, cols = x.shape if x.dim() == 3 else (1, *x.shape)
    ld = x.stride(-2) if rows > 1 else max(x.stride(-2), cols)
    return code, count, x.stride(0) if count > 1 else rows * ld, rows, cols, ld


def _contiguous_batch(x3d):
    """_matrix of a contiguous (count, rows, cols) device tensor."""
    m = _matrix(x3d, (3,))
    if not x3d.is_contiguous():
        raise MtqError("expected a contiguous (count, rows, cols) device tensor")
    return m


def _as_device_matrix(t):
    """2-D device tensor → (tensor with contiguous rows, storage code, rows, cols, ld); other inner strides are copied.  A single
    column's stride means nothing (contiguous() keeps it, e.g. on the transpose of one row): it is set to 1 in place."""
    if t.dim() == 2 and t.stride(1) != 1:
        t = t.contiguous() if t.shape[1] > 1 else t.as_strided(t.shape, (t.stride(0), 1))
    code, _count, _stride, rows, cols, ld = _matrix(t, (2,))
    return t, code, rows, cols, ld


def _buffer(t, dtype, numel: int, name: str, device: bool = True) -> int:
    """The pointer of a buffer a launch reads or writes numel elements of, after checking it can: dtype, contiguity, size (a lower
    bound: callers pass views of grow-only storage) and, unless it is a host mirror, that it is device memory."""
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < numel or (device and not t.is_cuda):
        raise MtqError(f"{name} must be a contiguous {dtype} {'device ' if device else ''}tensor of at least {numel} elements")
    return t.data_ptr()


def _stream(s):
    """The HIP handle of a torch stream; None is the null stream."""
    return None if s is None else s.cuda_stream


def _format_codes(formats):
    return (ctypes.c_int * len(formats))(*[MIXED_TILE_FORMATS.index(f) for f in formats])


def _columns(out) -> dict:
    """The columns of mtq_columns_from_sums' nine doubles."""
    return {"pcc": out[0], "mae": out[1], "atol": out[2], "sums": tuple(out[3:9])}


def to_device_2d(x, device=None):
    """Host ndarray / torch tensor of any rank → (2-D device tensor, shape_info) following the 2-D
    flatten of compression_algorithms/tile_utils.py:91-107.  bf16 stays bf16, everything else → fp32."""
    torch = _torch()
    device = device or torch.device("cuda", torch.cuda.current_device())
    if isinstance(x, np.ndarray) or np.isscalar(x):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        if np.ndim(x) == 0:
            t = t.reshape(())
    else:
        t = x
        if t.dtype not in (torch.bfloat16, torch.float32):
            t = t.to(torch.float32)
    t = t.to(device, non_blocking=True)
    if t.dim() == 0:
        return t.reshape(1, 1), ("scalar", tuple(t.shape))
    if t.dim() == 1:
        n = t.shape[0]
        h = -(-n // TILE)
        d = torch.zeros((h, TILE), dtype=t.dtype, device=device)
        d.view(-1)[:n] = t
        return d, ("vector", n)
    shape = tuple(t.shape)
    return t.reshape(-1, shape[-1]).contiguous(), ("nd", shape)


def unflatten(y2d, shape_info):
    """Inverse of to_device_2d's flatten (tile_utils.py:123-131) for torch or numpy 2-D arrays."""
    kind, v = shape_info
    if kind == "scalar":
        return y2d.reshape(())
    if kind == "vector":
        return y2d.reshape(-1)[:v]
    return y2d.reshape(v)


def tile_stats(x2d, mask: int, out=None):
    """K1 on a 2-D device tensor → device float64 [tiles, 2+5F] (async on the current stream)."""
    torch = _torch()
    require_gpu()
    x2d, code, rows, cols, ld = _as_device_matrix(x2d)
    th, tw = tiles_hw(rows, cols)
    rec = record_doubles(mask)
    if out is None:
        out = torch.empty((th * tw, rec), dtype=torch.float64, device=x2d.device)
    check(lib().mtq_tile_stats(x2d.data_ptr(), code, rows, cols, ld, mask, out.data_ptr(), _stream_ptr()))
    return out


def tile_stats_batched(x3d, mask: int, out=None):
    """K1 over a (count, rows, cols) contiguous device tensor in one launch → [count, tiles, rec]."""
    torch = _torch()
    require_gpu()
    code, count, stride, rows, cols, ld = _contiguous_batch(x3d)
    th, tw = tiles_hw(rows, cols)
    rec = record_doubles(mask)
    if out is None:
        out = torch.empty((count, th * tw, rec), dtype=torch.float64, device=x3d.device)
    check(lib().mtq_tile_stats_batched(x3d.data_ptr(), code, count, stride, rows, cols, ld, mask, out.data_ptr(), _stream_ptr()))
    return out


RAGGED_MAX = 24   # include/mtq.h MTQ_RAGGED_MAX


class MtqMatrix(ctypes.Structure):
    """include/mtq.h MtqMatrix: one matrix of a ragged batch (device pointer, leading dimension in elements)."""
    _fields_ = [("x", ctypes.c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("ld", ctypes.c_int64)]


def ragged_matrices(mats):
    """(MtqMatrix array, storage code, tiles per matrix) of 2-D device tensors of one storage type with contiguous rows."""
    if not 0 < len(mats) <= RAGGED_MAX:
        raise MtqError(f"a ragged batch holds 1..{RAGGED_MAX} matrices")
    arr = (MtqMatrix * len(mats))()
    codes, tiles = set(), []
    for j, m in enumerate(mats):
        code, _count, _stride, rows, cols, ld = _matrix(m, (2,))
        codes.add(code)
        if len(codes) > 1 or m.device != mats[0].device:
            raise MtqError("a ragged batch is 2-D tensors of one storage type on one device with contiguous rows")
        arr[j] = MtqMatrix(m.data_ptr(), rows, cols, ld)
        th, tw = tiles_hw(rows, cols)
        tiles.append(th * tw)
    return arr, code, tiles


def tile_stats_ragged(mats, mask: int, out=None):
    """K1 over matrices of ANY shapes (one storage type) in one launch (mtq_tile_stats_ragged) → [sum of their tiles, rec], matrix j's
    tiles row-major behind matrix j-1's."""
    torch = _torch()
    require_gpu()
    arr, code, tiles = ragged_matrices(mats)
    if out is None:
        out = torch.empty((sum(tiles), record_doubles(mask)), dtype=torch.float64, device=mats[0].device)
    check(lib().mtq_tile_stats_ragged(arr, len(mats), code, mask, out.data_ptr(), _stream_ptr()))
    return out


def tile_stats_partial(x3d, layout_mask: int, full_mask: int, sums_mask: int, out=None):
    """K1 over a (count, rows, cols) device tensor with only part of every record promised (mtq_tile_stats_partial): the five statistics of
    the formats in full_mask, Σy, Σy², Σxy of those in sums_mask; the rest of the layout is unspecified → [count, tiles, rec(layout)]."""
    torch = _torch()
    require_gpu()
    code, count, stride, rows, cols, ld = _contiguous_batch(x3d)
    th, tw = tiles_hw(rows, cols)
    if out is None:
        out = torch.empty((count, th * tw, record_doubles(layout_mask)), dtype=torch.float64, device=x3d.device)
    check(lib().mtq_tile_stats_partial(x3d.data_ptr(), code, count, stride, rows, cols, ld, layout_mask, full_mask, sums_mask,
                                       out.data_ptr(), _stream_ptr()))
    return out


def tile_stats_partial_begin(x3d, layout_mask: int, full_mask: int, sums_mask: int, out, mark) -> int:
    """mtq_tile_stats_partial_begin on the current stream (the exact-integer kernel alone) → the launch id tile_stats_partial_end wants.
    mark: int32 device tensor of one element that stays the caller's until _end has run."""
    code, count, stride, rows, cols, ld = _contiguous_batch(x3d)
    lid = ctypes.c_uint32(0)
    check(lib().mtq_tile_stats_partial_begin(x3d.data_ptr(), code, count, stride, rows, cols, ld, layout_mask, full_mask, sums_mask,
                                             out.data_ptr(), mark.data_ptr(), ctypes.byref(lid), _stream_ptr()))
    return int(lid.value)


def tile_stats_partial_begin_early(x3d, layout_mask: int, full_mask: int, sums_mask: int, out, mark, rank, cutoff: int) -> int:
    """mtq_tile_stats_partial_begin_early: tile_stats_partial_begin that also writes, for every tile with rank[tile] < cutoff (rank: int32 /
    uint32 device tensor over a tensor's tiles, scan_rank_device), what tile_stats_listed would write for it.  cutoff 0: the plain launch."""
    code, count, stride, rows, cols, ld = _matrix(x3d, (3,))   # views too: the entry checks the alignment of ld and the batch stride
    th, tw = tiles_hw(rows, cols)
    if rank.numel() < th * tw or rank.element_size() != 4:
        raise ValueError("rank must hold one 32-bit entry per tile of a tensor")
    lid = ctypes.c_uint32(0)
    check(_entry("mtq_tile_stats_partial_begin_early")(x3d.data_ptr(), code, count, stride, rows, cols, ld, layout_mask, full_mask, sums_mask,
                                                       out.data_ptr(), mark.data_ptr(), ctypes.byref(lid), rank.data_ptr(), int(cutoff), _stream_ptr()))
    return int(lid.value)


def tile_stats_partial_end(x3d, layout_mask: int, stats, mark, launch_id: int) -> None:
    """mtq_tile_stats_partial_end on the current stream: the literal fix-up of the tiles that launch could not take (usually none)."""
    code, count, stride, rows, cols, ld = _matrix(x3d, (3,))
    check(lib().mtq_tile_stats_partial_end(x3d.data_ptr(), code, count, stride, rows, cols, ld, layout_mask, stats.data_ptr(),
                                           mark.data_ptr(), int(launch_id), _stream_ptr()))


K1_BF16, K1_DIRECT = 0, 1   # include/mtq.h MTQ_K1_BF16, MTQ_K1_DIRECT


def k1_grid(kind: int, total: int, cus: int, waves_per_simd: int = -1, units_per_wave: int = -1) -> tuple[int, int, int]:
    """mtq_debug_k1_grid (a host function): (blocks, per-wave quota as the kernel gets it, counter groups) of a K1 launch over `total`
    units (K1_BF16) or tiles (K1_DIRECT) on `cus` compute units; negative switches stand for this process's own."""
    out = (ctypes.c_int64 * 3)()
    check(_entry("mtq_debug_k1_grid")(int(kind), int(total), int(cus), int(waves_per_simd), int(units_per_wave), out))
    return int(out[0]), int(out[1]), int(out[2])


def k1_waves_per_block(kind: int) -> int:
    """Waves in a block of that kernel, read off the grid of 64 units on a device with room for all of them (blocks = ceil(64 / W))."""
    return 64 // k1_grid(kind, 64, 4096, 8, 0)[0]


def k1_regime(kind: int, total: int, cus: int, waves_per_simd: int = -1, units_per_wave: int = -1) -> str:
    """The regime of that launch (csrc/mtq_error.hpp k1_grid): 'resident' (every unit has a wave of its own), 'quota' (waves retire
    after their quota, the grid is what fits the chip), 'oversubscribed' (more blocks than fit), or 'persistent' (more units than
    waves and no quota: units_per_wave 0)."""
    blocks, quota, _groups = k1_grid(kind, total, cus, waves_per_simd, units_per_wave)
    if quota == 0:
        return "resident" if blocks * k1_waves_per_block(kind) >= total else "persistent"
    resident = k1_grid(kind, total, cus, waves_per_simd, 0)[0]
    return "quota" if blocks == resident else "oversubscribed"


def work_counters_nonzero() -> int:
    """mtq_debug_work_counters: synchronises the current device; how many K1 claim counters and completion words of its ring are not zero
    (0 between launches, whatever ran before)."""
    n = ctypes.c_int64(-1)
    check(_entry("mtq_debug_work_counters")(ctypes.byref(n)))
    return int(n.value)


def quantize(x2d, fmt: str, out=None):
    """K2 on a 2-D device tensor → device float32 (rows, cols); the proxies mxfp4 / nvfp4 elementwise (csrc/mtq_fp4_proxy.hip)."""
    torch = _torch()
    require_gpu()
    if fmt not in QUANTIZE_CODE:
        raise ValueError(f"Unsupported weight format: {fmt}")
    x2d, code, rows, cols, ld = _as_device_matrix(x2d)
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x2d.device)
    check(lib().mtq_quantize(x2d.data_ptr(), code, rows, cols, ld, QUANTIZE_CODE[fmt], out.data_ptr(), out.stride(0), _stream_ptr()))
    return out


PROXY_MAX_COUNT = 65535   # matrices per mtq_fp4_proxy_sums launch (the grid's y dimension)


def fp4_proxy_sums(x, formats, out=None, scratch=None):
    """FP4P (mtq_fp4_proxy_sums) on the current stream: one read of a (rows, cols) or (count, rows, cols) device tensor with contiguous
    rows → float64 [2, 7] / [count, 2, 7] device sums (Σx, Σx², Σy, Σy², Σxy, Σ|x−y|, max|x−y|) of the proxies, slot 0 mxfp4, slot 1
    nvfp4; the slot of a proxy not in `formats` is zero.  The tensor is checked before any pointer is taken.  A batch of more than
    PROXY_MAX_COUNT matrices takes one launch per PROXY_MAX_COUNT of them, in order on the stream, sharing one chunk's scratch; the
    matrices are independent, so each gets the bits it gets alone."""
    code, count, stride, rows, cols, ld = _matrix(x)
    bad = [f for f in formats if f not in PROXY_FORMATS]
    if bad or not formats:
        raise MtqError(f"fp4_proxy_sums takes a non-empty subset of {PROXY_FORMATS}, got {list(formats)}")
    mask = sum(1 << PROXY_FORMATS.index(f) for f in set(formats))
    torch = _torch()
    require_gpu()
    fn = _entry("mtq_fp4_proxy_sums")
    need = int(_entry("mtq_fp4_proxy_scratch_doubles")(min(count, PROXY_MAX_COUNT), rows, cols))
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.float64, device=x.device)
    else:
        _buffer(scratch, torch.float64, need, "scratch")
    if out is None:
        out = torch.zeros((count, 2, 7), dtype=torch.float64, device=x.device)
    else:
        _buffer(out, torch.float64, count * 14, "out")
    x_ptr, out_ptr, esz = x.data_ptr(), out.data_ptr(), x.element_size()
    for m0 in range(0, count, PROXY_MAX_COUNT):
        n = min(PROXY_MAX_COUNT, count - m0)
        check(fn(x_ptr + m0 * stride * esz, code, n, stride, rows, cols, ld, mask, out_ptr + m0 * 14 * 8, scratch.data_ptr(), need,
                 _stream_ptr()))
    return out if x.dim() == 3 else out[0]


def fp4_proxy_columns(x, formats, elem_count: float | None = None) -> list:
    """fmt → (pcc, mae, atol) of each proxy in `formats` for every matrix of x (a list of dicts, one per matrix), from one
    fp4_proxy_sums launch; elem_count defaults to rows × cols (a vector's zero padding adds nothing to the sums)."""
    from .pipeline_common import gated_pcc

    s = fp4_proxy_sums(x, formats)
    host = s.reshape(-1, 2, 7).cpu().numpy()
    n = float(elem_count if elem_count is not None else x.shape[-1] * x.shape[-2])
    out = []
    for m, sums in enumerate(host):
        xm = x[m] if x.dim() == 3 else x
        cols = {}
        for f in formats:
            c = columns_from_sums(sums[PROXY_FORMATS.index(f)], n)
            pcc = gated_pcc(c["pcc"], c["sums"], n, xm, lambda: quantize(xm, f))
            cols[f] = (pcc, c["mae"], c["atol"])
        out.append(cols)
    return out


def _entry(name: str):
    """An optional symbol of the library (SIGNATURES), or MtqError if this build lacks it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise MtqError(f"{LIB_PATH} has no {name}: {_REBUILD}")
    return fn


_transposed_entry = _entry   # its earlier name, which the tests of the optional symbols still use


def tile_stats_transposed(x, mask: int, out=None):
    """K1T (mtq_tile_stats_transposed) on the current stream: the K1 records of Xᵀ for a (rows, cols) or (count, rows, cols) device tensor X
    with contiguous rows, read in place → float64 [tiles] / [count, tiles] × rec, tiles numbered row-major over Xᵀ's grid
    (element (r, c) of X in tile (c // 32) * ceil(rows / 32) + r // 32)."""
    code, count, stride, rows, cols, ld = _matrix(x)
    torch = _torch()
    require_gpu()
    fn = _entry("mtq_tile_stats_transposed")
    th_t, tw_t = tiles_hw(cols, rows)
    rec = record_doubles(mask)
    if out is None:
        out = torch.empty((count, th_t * tw_t, rec), dtype=torch.float64, device=x.device)
    check(fn(x.data_ptr(), code, count, stride, rows, cols, ld, mask, out.data_ptr(), _stream_ptr()))
    return out if x.dim() == 3 else out[0]


def quantize_transposed(x2d, fmt: str, out=None):
    """K2T (mtq_quantize_transposed) on the current stream: (K2 of Xᵀ)ᵀ for a 2-D device tensor with contiguous rows → float32, X's shape."""
    code, _count, _stride, rows, cols, ld = _matrix(x2d, (2,))
    torch = _torch()
    if fmt not in FMT_CODE:
        raise ValueError(f"Unsupported weight format: {fmt}")
    require_gpu()
    fn = _entry("mtq_quantize_transposed")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x2d.device)
    check(fn(x2d.data_ptr(), code, rows, cols, ld, FMT_CODE[fmt], out.data_ptr(), out.stride(0), _stream_ptr()))
    return out


def apply_assignment_transposed(x, assignment, out=None):
    """K3T (mtq_apply_assignment_transposed) on the current stream: (K3 of Xᵀ with `assignment`)ᵀ for a (rows, cols) or (count, rows, cols)
    device tensor X with contiguous rows, read in place → float32, X's shape.  assignment: int8 numpy array or device tensor with
    ceil(cols / 32) × ceil(rows / 32) entries per matrix (Xᵀ's grid, K1T's numbering)."""
    code, count, stride, rows, cols, ld = _matrix(x)
    torch = _torch()
    require_gpu()
    fn = _entry("mtq_apply_assignment_transposed")
    th_t, tw_t = tiles_hw(cols, rows)
    if isinstance(assignment, np.ndarray):
        assignment = torch.from_numpy(np.ascontiguousarray(assignment, dtype=np.int8)).to(x.device)
    a = assignment.to(device=x.device, dtype=torch.int8).contiguous()
    if a.numel() != count * th_t * tw_t:
        raise MtqError(f"assignment has {a.numel()} entries, the transposed grid has {count}x{th_t}x{tw_t} tiles")
    if out is None:
        out = torch.empty((count, rows, cols), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (count, rows, cols) or not out.is_contiguous() or out.device != x.device:
        raise MtqError("out must be a contiguous float32 device tensor of X's shape")
    check(fn(x.data_ptr(), code, count, stride, rows, cols, ld, a.data_ptr(), out.data_ptr(), cols, _stream_ptr()))
    return out if x.dim() == 3 else out[0]


OE_SLOTS = ("bf16", "bfp8", "bfp4", "bfp2", "map", "fp0", "recorded")  # include/mtq.h MTQ_OE_* (rows of the sums array)


X_FORMATS = ("bf16", "bfp8", "bfp4", "bfp2")   # activation formats of the LOE (mtq_quantize_rows_bf16); fp0 and the proxies are not


def quantize_rows_bf16(x, fmt: str, out=None):
    """LOE activation pre-pass (mtq_quantize_rows_bf16) on the current stream: Q(X) of an (m, k) bf16 device tensor with contiguous rows in
    the row layout, as bf16 (the upper halves of K2's float32 y).  out: an (m, k) bf16 device tensor with contiguous rows (allocated when
    None), not overlapping x."""
    if fmt not in X_FORMATS:
        raise ValueError(f"Unsupported activation format: {fmt} (one of {', '.join(X_FORMATS)})")
    torch = _torch()
    _code, _count, _stride, m, k, ld = _matrix(x, (2,))
    if x.dtype != torch.bfloat16:
        raise MtqError(f"x must be bfloat16, got {x.dtype}")
    require_gpu()
    fn = _entry("mtq_quantize_rows_bf16")
    if out is None:
        out = torch.empty((m, k), dtype=torch.bfloat16, device=x.device)
    _code, _count, _stride, om, ok, ldy = _matrix(out, (2,))
    if out.dtype != torch.bfloat16 or (om, ok) != (m, k) or out.device != x.device:
        raise MtqError(f"out must be a ({m}, {k}) bfloat16 tensor with contiguous rows on x's device")
    check(fn(x.data_ptr(), m, k, ld, FMT_CODE[fmt], out.data_ptr(), ldy, _stream_ptr()))
    return out


def output_error(x, w, fmt_mask: int, sums, bias=None, assignment=None, recorded=None, scratch=None, xq=None):
    """LOE (mtq_output_error) on the current stream: ADDS the output-error sums of one M-chunk to `sums` (float64 device tensor
    [7, 7], zeroed by the caller once per op).  x: (m, k) bf16 device tensor with contiguous rows; w: (n, k) bf16 / float32 device
    tensor with contiguous rows; bias: float32 [n] or None; assignment: int8 map of w's 32×32 grid or None; recorded: (m, n) bf16 /
    float32 or None.  scratch: float64 device tensor of at least output_error_scratch(m, n) elements (allocated when None).
    xq: None, or the candidates' activations Q(X) — an (m, k) bf16 device tensor with contiguous rows (quantize_rows_bf16 of x) — which
    takes mtq_output_error_qx: R keeps x, every candidate but fp0 is fed xq."""
    return _output_error(x, w, fmt_mask, sums, bias, assignment, recorded, scratch, xq, False)


def output_error_transposed(x, w, fmt_mask: int, sums, bias=None, assignment=None, recorded=None, scratch=None, xq=None):
    """LOE in the transposed BFP layout (mtq_output_error_transposed): output_error with Ŵ_f = K2_f(wᵀ)ᵀ for the bfp8 / bfp4 / bfp2 bits
    (groups of 16 consecutive rows of one column) and `assignment` over wᵀ's grid, an int8 map of tiles_hw(k, n).  R, the bf16 slot,
    fp0 and `recorded` are those of output_error bit for bit.  xq: as output_error (None = W-only)."""
    return _output_error(x, w, fmt_mask, sums, bias, assignment, recorded, scratch, xq, True)


def _output_error(x, w, fmt_mask: int, sums, bias, assignment, recorded, scratch, xq, transposed: bool):
    torch = _torch()
    require_gpu()
    if transposed:
        fn = _entry("mtq_output_error_transposed")
    else:
        fn = _entry("mtq_output_error" if xq is None else "mtq_output_error_qx")
    _code, _count, _stride, m, k, ldx = _matrix(x, (2,))
    w_code, _count, _stride, n, kw, ldw = _matrix(w, (2,))
    if x.dtype != torch.bfloat16:
        raise MtqError(f"x must be bfloat16, got {x.dtype}")
    if kw != k:
        raise MtqError(f"x has {k} columns, w has {kw}")
    if sums.dtype != torch.float64 or tuple(sums.shape) != (len(OE_SLOTS), 7) or not sums.is_contiguous() or not sums.is_cuda:
        raise MtqError("sums must be a contiguous float64 device tensor of shape (7, 7)")
    bp = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != n or not bias.is_contiguous() or not bias.is_cuda:
            raise MtqError("bias must be a contiguous float32 device tensor of n elements")
        bp = bias.data_ptr()
    mp = 0
    if assignment is not None:
        th, tw = tiles_hw(k, n) if transposed else tiles_hw(n, k)
        if assignment.dtype != torch.int8 or assignment.numel() != th * tw or not assignment.is_contiguous() or not assignment.is_cuda:
            raise MtqError(f"assignment must be a contiguous int8 device tensor of {th}x{tw} entries")
        mp = assignment.data_ptr()
    rp, rdt, ldr = 0, 0, 0
    if recorded is not None:
        rdt, _count, _stride, rm, rn, ldr = _matrix(recorded, (2,))
        if (rm, rn) != (m, n):
            raise MtqError(f"recorded must be a ({m}, {n}) device tensor with contiguous rows")
        rp = recorded.data_ptr()
    qx = (0, 0) if transposed else ()
    if xq is not None:
        _code, _count, _stride, qm, qk, ldxq = _matrix(xq, (2,))
        if xq.dtype != torch.bfloat16 or (qm, qk) != (m, k) or xq.device != x.device:
            raise MtqError(f"xq must be a ({m}, {k}) bfloat16 tensor with contiguous rows on x's device")
        qx = (xq.data_ptr(), ldxq)
    need = output_error_scratch(m, n)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.float64, device=x.device)
    elif scratch.numel() < need:
        raise MtqError(f"scratch holds {scratch.numel()} doubles, the launch needs {need}")
    check(fn(x.data_ptr(), m, k, ldx, w.data_ptr(), w_code, n, ldw, bp, fmt_mask, mp, rp, rdt, ldr,
             sums.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream_ptr(), *qx))
    return sums


def output_error_scratch(m: int, n: int) -> int:
    """Doubles of scratch one mtq_output_error launch over m × n outputs needs."""
    return int(_entry("mtq_output_error_scratch_doubles")(m, n))


def gram_blocks(x, h, scratch=None):
    """Budget maps' Gram blocks (mtq_gram_blocks) on the current stream: ADDS the diagonal 32 × 32 blocks of XᵀX of one chunk to h.
    x: (m, k) bf16 device tensor with contiguous rows; h: contiguous float64 device tensor (ceil(k/32), 32, 32), zeroed by the caller
    once.  scratch: float64 device tensor of at least gram_blocks_scratch(m, k) elements (allocated when None)."""
    torch = _torch()
    _code, _count, _stride, m, k, ldx = _matrix(x, (2,))
    if x.dtype != torch.bfloat16:
        raise MtqError(f"x must be bfloat16, got {x.dtype}")
    nb = -(-k // TILE)
    if h.dtype != torch.float64 or tuple(h.shape) != (nb, TILE, TILE) or not h.is_contiguous() or not h.is_cuda or h.device != x.device:
        raise MtqError(f"h must be a contiguous float64 tensor of shape ({nb}, 32, 32) on x's device")
    require_gpu()
    fn = _entry("mtq_gram_blocks")
    need = gram_blocks_scratch(m, k)
    if scratch is None:
        scratch = torch.empty((max(need, 1),), dtype=torch.float64, device=x.device)
    elif scratch.dtype != torch.float64 or not scratch.is_contiguous() or not scratch.is_cuda or scratch.numel() < need:
        raise MtqError(f"scratch must be a contiguous float64 device tensor of at least {need} elements")
    check(fn(x.data_ptr(), m, k, ldx, h.data_ptr(), h.numel(), scratch.data_ptr(), scratch.numel(), _stream_ptr()))
    return h


def gram_blocks_scratch(m: int, k: int) -> int:
    """Doubles of scratch one mtq_gram_blocks launch over an (m, k) chunk needs."""
    return int(_entry("mtq_gram_blocks_scratch_doubles")(m, k))


def tile_error_tables(w, h, want_weight: bool = True):
    """Budget maps' tile error tables (mtq_tile_error_tables) on the current stream → (e_out, e_w or None), float64 device tensors
    [tiles, 4] indexed by MIXED_TILE_FORMATS code, tiles row-major over w's 32 × 32 grid.  w: (n, k) bf16 / float32 device tensor with
    contiguous rows; h: its Gram blocks, a contiguous float64 tensor (ceil(k/32), 32, 32) on w's device."""
    torch = _torch()
    w_code, _count, _stride, n, k, ldw = _matrix(w, (2,))
    th, tw = tiles_hw(n, k)
    if h.dtype != torch.float64 or tuple(h.shape) != (tw, TILE, TILE) or not h.is_contiguous() or not h.is_cuda or h.device != w.device:
        raise MtqError(f"h must be a contiguous float64 tensor of shape ({tw}, 32, 32) on w's device")
    require_gpu()
    fn = _entry("mtq_tile_error_tables")
    out = torch.empty((2 if want_weight else 1, th * tw, 4), dtype=torch.float64, device=w.device)
    check(fn(w.data_ptr(), w_code, n, k, ldw, h.data_ptr(), h.numel(), out[0].data_ptr(), out[1].data_ptr() if want_weight else 0,
             th * tw * 4, _stream_ptr()))
    return out[0], (out[1] if want_weight else None)


def tile_error_tables_transposed(w, h, want_weight: bool = True):
    """tile_error_tables in the transposed layout (mtq_tile_error_tables_transposed): Δ from groups of 16 consecutive rows of one column,
    tiles row-major over wᵀ's grid, tiles_hw(k, n).  Same arguments and h as tile_error_tables."""
    torch = _torch()
    w_code, _count, _stride, n, k, ldw = _matrix(w, (2,))
    th, tw = tiles_hw(k, n)
    if h.dtype != torch.float64 or tuple(h.shape) != (th, TILE, TILE) or not h.is_contiguous() or not h.is_cuda or h.device != w.device:
        raise MtqError(f"h must be a contiguous float64 tensor of shape ({th}, 32, 32) on w's device")
    require_gpu()
    fn = _entry("mtq_tile_error_tables_transposed")
    out = torch.empty((2 if want_weight else 1, th * tw, 4), dtype=torch.float64, device=w.device)
    check(fn(w.data_ptr(), w_code, n, k, ldw, h.data_ptr(), h.numel(), out[0].data_ptr(), out[1].data_ptr() if want_weight else 0,
             th * tw * 4, _stream_ptr()))
    return out[0], (out[1] if want_weight else None)


def tile_sq_error_batched(x, out=None):
    """The weight-space error tables of a batch (mtq_tile_sq_error_batched) on the current stream → float64 device tensor [count, tiles, 4]
    by MIXED_TILE_FORMATS code: Σ (K2_f(x) − x)² of every 32 × 32 tile, bit for bit tile_error_tables' e_w of each matrix.  x: a (rows,
    cols) or (count, rows, cols) bf16 / float32 device tensor with contiguous rows (a strided batch view is read in place)."""
    torch = _torch()
    code, count, stride, rows, cols, ld = _matrix(x)
    th, tw = tiles_hw(rows, cols)
    if count > 1 and stride < (rows - 1) * ld + cols:
        raise MtqError("the matrices of the batch overlap (stride(0) is shorter than a matrix)")
    require_gpu()
    fn = _entry("mtq_tile_sq_error_batched")
    if out is None:
        out = torch.empty((count, th * tw, 4), dtype=torch.float64, device=x.device)
    check(fn(x.data_ptr(), code, count, stride, rows, cols, ld, _buffer(out, torch.float64, count * th * tw * 4, "out"), _stream_ptr()))
    return out


def budget_allocate_scratch_bytes(tiles: int, n_seg: int) -> int:
    """Bytes of scratch one mtq_budget_allocate_device call over `tiles` tiles in `n_seg` segments needs."""
    return int(_entry("mtq_budget_allocate_scratch_bytes")(int(tiles), int(n_seg)))


BUDGET_STATUS_BELOW_FLOOR, BUDGET_STATUS_NON_FINITE = 1, 2   # include/mtq.h: mtq_budget_allocate_device's status


def budget_allocate_device(table, seg_first, formats, budget_bytes, scratch=None):
    """budget_maps.allocate on the device (mtq_budget_allocate_device) on the current stream, nothing read back → (maps int8 [tiles],
    counts int64 [n_seg, 4], status int32 [n_seg]) device tensors.  table: contiguous float64 device tensor [tiles, 4]; seg_first: int64
    device tensor [n_seg + 1], segment j = tiles seg_first[j] .. seg_first[j + 1] − 1; budget_bytes: float64 device tensor [n_seg];
    formats: the candidates (those outside MIXED_TILE_FORMATS are ignored, as allocate ignores them).  scratch: a uint8 device tensor of
    at least budget_allocate_scratch_bytes(tiles, n_seg) (allocated when None)."""
    torch = _torch()
    if table.dim() != 2 or table.shape[1] != 4:
        raise MtqError(f"table must be [tiles, 4], got {tuple(table.shape)}")
    T = int(table.shape[0])
    if seg_first.dim() != 1 or seg_first.numel() < 2:
        raise MtqError("seg_first must hold n_seg + 1 >= 2 entries")
    n_seg = int(seg_first.numel()) - 1
    mask = fmt_mask([f for f in formats if f in MIXED_TILE_FORMATS])
    if T <= 0 or not mask:
        raise MtqError("budget_allocate_device needs at least one tile and one mixed-tile format")
    if table.device != seg_first.device or table.device != budget_bytes.device:
        raise MtqError("table, seg_first and budget_bytes must be on one device")
    tp = _buffer(table, torch.float64, T * 4, "table")
    fp = _buffer(seg_first, torch.int64, n_seg + 1, "seg_first")
    bp = _buffer(budget_bytes, torch.float64, n_seg, "budget_bytes")
    require_gpu()
    fn = _entry("mtq_budget_allocate_device")
    need = budget_allocate_scratch_bytes(T, n_seg)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=table.device)
    sp = _buffer(scratch, torch.uint8, need, "scratch")
    maps = torch.empty((T,), dtype=torch.int8, device=table.device)
    counts = torch.empty((n_seg, 4), dtype=torch.int64, device=table.device)
    status = torch.empty((n_seg,), dtype=torch.int32, device=table.device)
    check(fn(tp, T, fp, n_seg, mask, bp, maps.data_ptr(), counts.data_ptr(), status.data_ptr(), sp, scratch.numel(), _stream_ptr()))
    return maps, counts, status


def gram_full(x, h, scratch=None):
    """GPTQ's full Gram matrix (mtq_gram_full) on the current stream: ADDS XᵀX of one chunk to h.  x: (m, k) bf16 device tensor with
    contiguous rows; h: contiguous float64 (k, k) tensor on x's device, zeroed by the caller once.  scratch: float64 device tensor of at
    least gram_full_scratch(m, k) elements (allocated when None)."""
    torch = _torch()
    _code, _count, _stride, m, k, ldx = _matrix(x, (2,))
    if x.dtype != torch.bfloat16:
        raise MtqError(f"x must be bfloat16, got {x.dtype}")
    if h.dtype != torch.float64 or tuple(h.shape) != (k, k) or not h.is_contiguous() or not h.is_cuda or h.device != x.device:
        raise MtqError(f"h must be a contiguous float64 tensor of shape ({k}, {k}) on x's device")
    require_gpu()
    fn = _entry("mtq_gram_full")
    need = gram_full_scratch(m, k)
    if scratch is None:
        scratch = torch.empty((max(need, 1),), dtype=torch.float64, device=x.device)
    elif scratch.dtype != torch.float64 or not scratch.is_contiguous() or not scratch.is_cuda or scratch.numel() < max(need, 1):
        raise MtqError(f"scratch must be a contiguous float64 device tensor of at least {max(need, 1)} elements")
    check(fn(x.data_ptr(), m, k, ldx, h.data_ptr(), h.numel(), scratch.data_ptr(), scratch.numel(), _stream_ptr()))
    return h


def gram_full_scratch(m: int, k: int) -> int:
    """Doubles of scratch one mtq_gram_full launch over an (m, k) chunk needs (0 when the block pairs alone fill the device)."""
    return int(_entry("mtq_gram_full_scratch_doubles")(m, k))


def gptq_sweep(w, u, codes, out=None, loss=None):
    """GPTQ's column sweep (mtq_gptq_sweep) on the current stream → (Ŵ float32 (n, k), loss float64 (n,)) device tensors.  w: (n, k)
    bf16 / float32 device tensor with contiguous rows; u: contiguous float64 (k, k) tensor on w's device (upper triangle read); codes:
    contiguous int8 (ceil(n/32), ceil(k/32)) device tensor of MIXED_TILE_FORMATS codes 0..3."""
    torch = _torch()
    w_code, _count, _stride, n, k, ldw = _matrix(w, (2,))
    th, tw = tiles_hw(n, k)
    if u.dtype != torch.float64 or tuple(u.shape) != (k, k) or not u.is_contiguous() or not u.is_cuda or u.device != w.device:
        raise MtqError(f"u must be a contiguous float64 tensor of shape ({k}, {k}) on w's device")
    if codes.dtype != torch.int8 or codes.numel() != th * tw or not codes.is_contiguous() or not codes.is_cuda or codes.device != w.device:
        raise MtqError(f"codes must be a contiguous int8 tensor of {th}x{tw} entries on w's device")
    if codes.numel() and (int(codes.min()) < 0 or int(codes.max()) > 3):
        raise MtqError("codes must be MIXED_TILE_FORMATS codes 0..3")
    require_gpu()
    fn = _entry("mtq_gptq_sweep")
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=w.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (n, k) or out.stride(1) != 1 or out.device != w.device:
        raise MtqError(f"out must be a float32 ({n}, {k}) tensor with contiguous rows on w's device")
    if loss is None:
        loss = torch.empty((n,), dtype=torch.float64, device=w.device)
    elif loss.dtype != torch.float64 or loss.numel() != n or not loss.is_contiguous() or loss.device != w.device:
        raise MtqError(f"loss must be a contiguous float64 tensor of {n} elements on w's device")
    need = int(_entry("mtq_gptq_sweep_scratch_doubles")(n, k))
    scratch = torch.empty((need,), dtype=torch.float64, device=w.device)
    check(fn(w.data_ptr(), w_code, n, k, ldw, u.data_ptr(), u.numel(), codes.data_ptr(), codes.numel(), out.data_ptr(), out.stride(0),
             loss.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream_ptr()))
    return out, loss


def apply_assignment(x2d, assignment, out=None):
    """K3: assignment is an int8 (tiles_h, tiles_w) numpy array or device tensor."""
    torch = _torch()
    require_gpu()
    x2d, code, rows, cols, ld = _as_device_matrix(x2d)
    th, tw = tiles_hw(rows, cols)
    if isinstance(assignment, np.ndarray):
        assignment = torch.from_numpy(np.ascontiguousarray(assignment, dtype=np.int8)).to(x2d.device)
    a = assignment.to(torch.int8).contiguous()
    if a.numel() != th * tw:
        raise MtqError(f"assignment has {a.numel()} entries, tensor has {th}x{tw} tiles")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x2d.device)
    check(lib().mtq_apply_assignment(x2d.data_ptr(), code, rows, cols, ld, a.data_ptr(), out.data_ptr(), out.stride(0), _stream_ptr()))
    return out


# ----------------------------------------------------------------------------- packed mixed-tile weights (csrc/mtq_packed.hip)

PACKED_TILE_BYTES = (2048, 1088, 576, 320)   # include/mtq.h: blob bytes by map code (bf16, bfp8, bfp4, bfp2)


def packed_offsets(amap) -> np.ndarray:
    """mtq_packed_offsets (a host function: no GPU): uint32[tiles + 1], the exclusive prefix sum of the blob sizes in units of 64 bytes.
    A code outside 0..3 is refused."""
    a = np.ascontiguousarray(np.asarray(amap, dtype=np.int8).reshape(-1))
    if a.size == 0:
        raise MtqError("the map has no tiles")
    out = np.empty(a.size + 1, dtype=np.uint32)
    check(_entry("mtq_packed_offsets")(a.ctypes.data, a.size, out.ctypes.data))
    return out


class PackedTables:
    """What the packed kernels read beside the stream: the int8 map (1 B per tile) and the uint32 offsets, on the device, checked on the
    host first — the map's codes are 0..3 and the offsets are those of the map, so `nbytes` is the stream's exact length and a launch
    that is given at least that many bytes stays inside them.  map_dev: contiguous int8 [tiles]; offsets_dev: contiguous int32 [tiles + 1]
    holding the uint32 words (torch has no arithmetic on uint32; nothing here needs any)."""

    def __init__(self, amap, map_dev, offsets_dev):
        torch = _torch()
        a = np.asarray(amap)
        if a.ndim != 2 or a.size == 0:
            raise MtqError("the map must be a 2-D (tiles_h, tiles_w) array")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 3):
            raise MtqError("map codes must be MIXED_TILE_FORMATS codes 0..3 (bf16, bfp8, bfp4, bfp2)")
        self.tiles_h, self.tiles_w = (int(v) for v in a.shape)
        tiles = self.tiles_h * self.tiles_w
        self.nbytes = int(np.asarray(PACKED_TILE_BYTES, dtype=np.int64)[a.reshape(-1).astype(np.int64)].sum())
        self.map_ptr = _buffer(map_dev, torch.int8, tiles, "the device map")
        self.offsets_ptr = _buffer(offsets_dev, torch.int32, tiles + 1, "the device offsets")
        self.map_dev, self.offsets_dev = map_dev, offsets_dev

    @classmethod
    def on_device(cls, amap, offsets=None, device=None):
        """The tables of a host map (and its offsets, computed when not given) copied to `device`."""
        torch = _torch()
        require_gpu()
        device = device or torch.device("cuda", torch.cuda.current_device())
        a = np.ascontiguousarray(np.asarray(amap, dtype=np.int8))
        own = packed_offsets(a)
        if offsets is not None and not np.array_equal(np.asarray(offsets, dtype=np.uint32).reshape(-1), own):
            raise MtqError("the offsets are not those of the map")
        return cls(a, torch.from_numpy(a.reshape(-1).copy()).to(device), torch.from_numpy(own.view(np.int32).copy()).to(device))


def _packed_out_code(dtype) -> int:
    torch = _torch()
    if dtype == torch.float32:
        return DTYPE_F32
    if dtype == torch.bfloat16:
        return DTYPE_BF16
    raise MtqError(f"the output type must be torch.float32 or torch.bfloat16, got {dtype}")


def _packed_stream_ptr(stream):
    return _stream_ptr() if isinstance(stream, str) else _stream(stream)


def _packed_stream(data, tables, name="data") -> int:
    torch = _torch()
    ptr = _buffer(data, torch.uint8, tables.nbytes, name)
    if data.data_ptr() % 16:
        raise MtqError(f"{name} must be 16-byte aligned")
    return ptr


def pack_tiles(x2d, tables: PackedTables, out=None, stream="current"):
    """mtq_pack_tiles on the current stream (or a torch stream; None is the null stream): a (rows, cols) bf16 / float32 device tensor with contiguous rows → the packed stream, a
    uint8 device tensor of tables.nbytes bytes."""
    torch = _torch()
    code, _count, _stride, rows, cols, ld = _matrix(x2d, (2,))
    if tiles_hw(rows, cols) != (tables.tiles_h, tables.tiles_w):
        raise MtqError(f"the map is {tables.tiles_h}x{tables.tiles_w} tiles, the tensor has {'x'.join(map(str, tiles_hw(rows, cols)))}")
    fn = _entry("mtq_pack_tiles")
    if out is None:
        require_gpu()
        out = torch.empty((tables.nbytes,), dtype=torch.uint8, device=x2d.device)
    ptr = _packed_stream(out, tables, "out")
    check(fn(x2d.data_ptr(), code, rows, cols, ld, tables.map_ptr, tables.offsets_ptr, ptr, tables.nbytes, _packed_stream_ptr(stream)))
    return out


def unpack_tiles(data, tables: PackedTables, rows: int, cols: int, dtype=None, out=None, stream="current"):
    """mtq_unpack_tiles on the current stream → a (rows, cols) device tensor: float32 (the bits K3 writes) or bfloat16 (exact)."""
    torch = _torch()
    dtype = dtype or torch.float32
    code = _packed_out_code(dtype)
    if tiles_hw(rows, cols) != (tables.tiles_h, tables.tiles_w):
        raise MtqError(f"the map is {tables.tiles_h}x{tables.tiles_w} tiles, a {rows}x{cols} tensor has {'x'.join(map(str, tiles_hw(rows, cols)))}")
    ptr = _packed_stream(data, tables)
    fn = _entry("mtq_unpack_tiles")
    if out is None:
        require_gpu()
        out = torch.empty((rows, cols), dtype=dtype, device=data.device)
    elif out.dtype != dtype or out.dim() != 2 or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or not out.is_cuda:
        raise MtqError(f"out must be a {dtype} ({rows}, {cols}) device tensor with contiguous rows")
    ldy = out.stride(0) if rows > 1 else max(out.stride(0), cols)
    check(fn(ptr, tables.nbytes, tables.map_ptr, tables.offsets_ptr, rows, cols, out.data_ptr(), code, ldy, _packed_stream_ptr(stream)))
    return out


PACKED_BATCH_MAX_TILES = 0xFFFFFFFF // 32   # include/mtq.h MTQ_PACKED_BATCH_MAX_TILES: a tensor's stream must fit 32-bit units


def _batch_tables(maps_dev, offsets_dev, bases_dev, count: int, tiles: int):
    """The pointers of a batch's device tables after checking their types and sizes: maps int8 [count * tiles], offsets int32
    [count * (tiles + 1)] holding the uint32 words, bases int64 [count + 1] holding the uint64 words."""
    torch = _torch()
    return (_buffer(maps_dev, torch.int8, count * tiles, "the device maps"), _buffer(offsets_dev, torch.int32, count * (tiles + 1), "the device offsets"),
            _buffer(bases_dev, torch.int64, count + 1, "the device bases"))


def _arena(data, count: int, tiles: int, name: str) -> int:
    """The pointer of a batch's arena: uint8, contiguous, on the device, 16-byte aligned and no shorter than the smallest streams the
    batch can have (the kernels check every blob against the arena's real length themselves)."""
    ptr = _buffer(data, _torch().uint8, count * tiles * PACKED_TILE_BYTES[3], name)
    if data.data_ptr() % 16:
        raise MtqError(f"{name} must be 16-byte aligned")
    return ptr


def packed_offsets_device(maps_dev, count: int, tiles: int, stream="current"):
    """mtq_packed_offsets_batched on the current stream: `count` maps of `tiles` int8 codes each, contiguous on the device →
    (offsets int32 [count, tiles + 1] holding the uint32 words, row i what packed_offsets gives for map i; bases int64 [count + 1], the
    exclusive prefix sum of the tensors' totals in units of 64 bytes; bad int32 [count], the codes outside 0..3 per map).  Nothing is
    read back: the caller looks at `bad` before it trusts a row."""
    torch = _torch()
    count, tiles = int(count), int(tiles)
    if count <= 0 or tiles <= 0:
        raise MtqError("count and tiles must be positive")
    if tiles > PACKED_BATCH_MAX_TILES:
        raise MtqError("too many tiles: a tensor's stream must fit 32-bit units")
    ptr = _buffer(maps_dev, torch.int8, count * tiles, "the device maps")
    fn = _entry("mtq_packed_offsets_batched")
    require_gpu()
    offsets = torch.empty((count, tiles + 1), dtype=torch.int32, device=maps_dev.device)
    bases = torch.empty((count + 1,), dtype=torch.int64, device=maps_dev.device)
    bad = torch.empty((count,), dtype=torch.int32, device=maps_dev.device)
    check(fn(ptr, count, tiles, offsets.data_ptr(), bases.data_ptr(), bad.data_ptr(), _packed_stream_ptr(stream)))
    return offsets, bases, bad


def pack_tiles_batched(x3d, maps_dev, offsets_dev, bases_dev, out, stream="current"):
    """mtq_pack_tiles_batched on the current stream: a (count, rows, cols) bf16 / float32 device tensor with contiguous rows (any row
    pitch and matrix stride: views are read in place) → the arena `out`, a uint8 device tensor of 64 * bases[count] bytes, tensor i's
    stream at byte 64 * bases[i]."""
    code, count, stride, rows, cols, ld = _matrix(x3d, (3,))
    th, tw = tiles_hw(rows, cols)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    fn = _entry("mtq_pack_tiles_batched")
    ptr = _arena(out, count, th * tw, "out")
    check(fn(x3d.data_ptr(), code, count, rows, cols, ld, stride, pm, po, pb, ptr, out.numel(), _packed_stream_ptr(stream)))
    return out


def unpack_tiles_batched(data, maps_dev, offsets_dev, bases_dev, count: int, rows: int, cols: int, dtype=None, out=None, stream="current"):
    """mtq_unpack_tiles_batched on the current stream: the arena → a (count, rows, cols) device tensor, float32 (the bits K3 writes) or
    bfloat16 (exact).  out: a tensor of that shape and type with contiguous rows; what lies outside rows × cols of a pitched view stays."""
    torch = _torch()
    dtype = dtype or torch.float32
    code = _packed_out_code(dtype)
    count, rows, cols = int(count), int(rows), int(cols)
    th, tw = tiles_hw(rows, cols)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    ptr = _arena(data, count, th * tw, "data")
    fn = _entry("mtq_unpack_tiles_batched")
    if out is None:
        require_gpu()
        out = torch.empty((count, rows, cols), dtype=dtype, device=data.device)
    elif out.dtype != dtype or out.dim() != 3 or tuple(out.shape) != (count, rows, cols) or out.stride(2) != 1 or not out.is_cuda:
        raise MtqError(f"out must be a {dtype} ({count}, {rows}, {cols}) device tensor with contiguous rows")
    _code, _count, stride, _rows, _cols, ldy = _matrix(out, (3,))
    check(fn(ptr, data.numel(), pm, po, pb, count, rows, cols, out.data_ptr(), code, ldy, stride, _packed_stream_ptr(stream)))
    return out


# The product entries below come in twins: one for a packed (n, k) weight (packed_linear*, packed_glu*) and one for a packed (k, n)
# matrix (packed_matmul*, packed_glu_matmul*).  A twin pair shares one body, told apart by `kn`; what else differs between two
# entries of a body is an argument of it, named where it is passed.

def _has(names) -> bool:
    """Whether this build of the library binds every one of `names` (optional symbols: an older build of the same version lacks them)."""
    return all(getattr(lib(), name, None) is not None for name in names)


def _workspace_size(name: str, *args) -> int:
    """A size function of the library (a host function: no GPU) on int arguments; its (size_t)-1 is the library's refusal."""
    size = int(_entry(name)(*map(int, args)))
    if size == ctypes.c_size_t(-1).value:
        raise MtqError(f"libmtq_hip error -1: {lib().mtq_last_error().decode()}")
    return size


def _packed_out(out, rows: int, cols: int, out_dtype, device, zeros: bool = False):
    """`out` checked, or a new (rows, cols) tensor → (out, ldy)."""
    torch = _torch()
    if out is None:
        require_gpu()
        out = (torch.zeros if zeros else torch.empty)((rows, cols), dtype=out_dtype, device=device)
    elif out.dtype != out_dtype or out.dim() != 2 or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or not out.is_cuda:
        raise MtqError(f"out must be a {out_dtype} ({rows}, {cols}) device tensor with contiguous rows")
    return out, (out.stride(0) if rows > 1 else max(out.stride(0), cols))


def _packed_workspace(workspace, need: int, device):
    """`workspace` checked, or a new one of `need` bytes → (pointer, bytes)."""
    torch = _torch()
    if workspace is None:
        require_gpu()
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    ws_ptr = _buffer(workspace, torch.uint8, need, "workspace")
    if workspace.data_ptr() % 16:
        raise MtqError("workspace must be 16-byte aligned")
    return ws_ptr, int(workspace.numel())


def _grid_error(tables, n: int, k: int, kn: bool, side: str = "") -> MtqError:
    """The tables' tile grid is not the operand's: an (n, k) weight's, or with `kn` a (k, n) matrix's."""
    rows, cols, noun = (k, n, "matrix") if kn else (n, k, "weight")
    own = "x".join(map(str, tiles_hw(rows, cols)))
    return MtqError(f"the {side}map is {tables.tiles_h}x{tables.tiles_w} tiles, a {rows}x{cols} {noun} has {own}")


def _packed_product_call(name, kn, empty, x, data, tables, n, bias, out_dtype, out, stream, size=None, split=0, workspace=None, size_first=False):
    """The checks and the call the single-tensor product entries share.  empty: which of "m" and "n" being 0 ends here with the empty
    `out` ("" : the library's refusal of empty operands reaches the caller).  size: a skinny entry's own size function, which makes
    the call one with m <= 32, a split and a workspace; size_first: it is asked before `out` is looked at."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code = _packed_out_code(out_dtype)
    x_code, _count, _stride, m, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    if size is not None and m > PACKED_SKINNY_MAX_M:
        raise MtqError(f"the skinny kernel takes m <= {PACKED_SKINNY_MAX_M}, got m = {m}")
    if (tiles_hw(k, n) if kn else tiles_hw(n, k)) != (tables.tiles_h, tables.tiles_w):
        raise _grid_error(tables, n, k, kn)
    ptr = _packed_stream(data, tables)
    bias_ptr = None if bias is None else _buffer(bias, torch.float32, n, "bias")
    need = size(m, n, k, split) if size_first else None
    fn = _entry(name)
    out, ldy = _packed_out(out, m, n, out_dtype, x.device)
    if (m == 0 and "m" in empty) or (n == 0 and "n" in empty):   # the entry refuses empty operands: they end here
        return out
    more = ()
    if size is not None:
        need = size(m, n, k, split) if need is None else need
        more = (int(split), *(_packed_workspace(workspace, need, x.device) if need else (None, 0)))
    check(fn(x.data_ptr(), m, k, ldx, ptr, tables.nbytes, tables.map_ptr, tables.offsets_ptr, n, bias_ptr, out.data_ptr(), code, ldy, *more,
             _packed_stream_ptr(stream)))
    return out


def packed_linear(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, stream="current"):
    """mtq_packed_linear on the current stream: Y = X·Ŵᵀ + b for an (m, k) bf16 device tensor X with contiguous rows and the packed
    (n, k) weight → (m, n) float32 or bfloat16 device tensor."""
    return _packed_product_call("mtq_packed_linear", False, "", x, data, tables, n, bias, out_dtype, out, stream)


def packed_linear_wide(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, stream="current"):
    """mtq_packed_linear_wide on the current stream: packed_linear's product, arguments and bits from the wide-block kernel (a
    128 x 128 block whose waves decode whole tiles), for m above the decode range.  Correct for any m; m = 0 or n = 0 gives the empty
    (m, n) tensor without a launch."""
    return _packed_product_call("mtq_packed_linear_wide", False, "mn", x, data, tables, n, bias, out_dtype, out, stream)


def has_packed_linear_wide() -> bool:
    """Whether this build of the library has mtq_packed_linear_wide (an optional symbol: an older build of the same version lacks it)."""
    return _has(("mtq_packed_linear_wide",))


PACKED_MATMUL = ("mtq_pack_tiles_transposed", "mtq_unpack_tiles_transposed", "mtq_packed_matmul")


def has_packed_matmul() -> bool:
    """Whether this build of the library has the transposed pack / unpack entries and mtq_packed_matmul (optional symbols: an older build
    of the same version lacks them)."""
    return _has(PACKED_MATMUL)


def pack_tiles_transposed(w2d, tables: PackedTables, out=None, stream="current"):
    """mtq_pack_tiles_transposed on the current stream: a (rows, cols) bf16 / float32 device tensor with contiguous rows, read in place →
    the packed stream of its (cols, rows) transpose, a uint8 device tensor of tables.nbytes bytes.  tables: over the transpose's grid."""
    torch = _torch()
    code, _count, _stride, rows, cols, ld = _matrix(w2d, (2,))
    if tiles_hw(cols, rows) != (tables.tiles_h, tables.tiles_w):
        raise MtqError(f"the map is {tables.tiles_h}x{tables.tiles_w} tiles, the transposed tensor has {'x'.join(map(str, tiles_hw(cols, rows)))}")
    fn = _entry("mtq_pack_tiles_transposed")
    if out is None:
        require_gpu()
        out = torch.empty((tables.nbytes,), dtype=torch.uint8, device=w2d.device)
    ptr = _packed_stream(out, tables, "out")
    check(fn(w2d.data_ptr(), code, rows, cols, ld, tables.map_ptr, tables.offsets_ptr, ptr, tables.nbytes, _packed_stream_ptr(stream)))
    return out


def unpack_tiles_transposed(data, tables: PackedTables, rows: int, cols: int, dtype=None, out=None, stream="current"):
    """mtq_unpack_tiles_transposed on the current stream: the stream of a (cols, rows) matrix → its (rows, cols) transpose as a device
    tensor, float32 (the bits K3T writes) or bfloat16 (exact).  What lies outside rows × cols of a pitched `out` stays."""
    torch = _torch()
    dtype = dtype or torch.float32
    code = _packed_out_code(dtype)
    rows, cols = int(rows), int(cols)
    if tiles_hw(cols, rows) != (tables.tiles_h, tables.tiles_w):
        raise MtqError(f"the map is {tables.tiles_h}x{tables.tiles_w} tiles, a transposed {rows}x{cols} tensor has {'x'.join(map(str, tiles_hw(cols, rows)))}")
    ptr = _packed_stream(data, tables)
    fn = _entry("mtq_unpack_tiles_transposed")
    if out is None:
        require_gpu()
        out = torch.empty((rows, cols), dtype=dtype, device=data.device)
    elif out.dtype != dtype or out.dim() != 2 or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or not out.is_cuda:
        raise MtqError(f"out must be a {dtype} ({rows}, {cols}) device tensor with contiguous rows")
    ldy = out.stride(0) if rows > 1 else max(out.stride(0), cols)
    check(fn(ptr, tables.nbytes, tables.map_ptr, tables.offsets_ptr, rows, cols, out.data_ptr(), code, ldy, _packed_stream_ptr(stream)))
    return out


PACKED_BATCH_TRANSPOSED = ("mtq_pack_tiles_transposed_batched", "mtq_unpack_tiles_transposed_batched")


def has_packed_batch_transposed() -> bool:
    """Whether this build of the library has the batched transposed pack / unpack entries (optional symbols: an older build of the same
    version lacks them)."""
    return _has(PACKED_BATCH_TRANSPOSED)


def pack_tiles_transposed_batched(w3d, maps_dev, offsets_dev, bases_dev, out, stream="current"):
    """mtq_pack_tiles_transposed_batched on the current stream: a (count, rows, cols) bf16 / float32 device tensor with contiguous rows
    (any row pitch and matrix stride: views are read in place) → the arena `out` of the streams of the (cols, rows) transposes, a uint8
    device tensor of 64 * bases[count] bytes, tensor i's stream at byte 64 * bases[i].  The tables are over the transposes' grid."""
    code, count, stride, rows, cols, ld = _matrix(w3d, (3,))
    th, tw = tiles_hw(cols, rows)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    fn = _entry("mtq_pack_tiles_transposed_batched")
    ptr = _arena(out, count, th * tw, "out")
    check(fn(w3d.data_ptr(), code, count, rows, cols, ld, stride, pm, po, pb, ptr, out.numel(), _packed_stream_ptr(stream)))
    return out


def unpack_tiles_transposed_batched(data, maps_dev, offsets_dev, bases_dev, count: int, rows: int, cols: int, dtype=None, out=None, stream="current"):
    """mtq_unpack_tiles_transposed_batched on the current stream: the arena of `count` (cols, rows) streams → the (count, rows, cols)
    transposes as a device tensor, float32 (the bits K3T writes) or bfloat16 (exact).  out: a tensor of that shape and type with
    contiguous rows; what lies outside rows × cols of a pitched view stays."""
    torch = _torch()
    dtype = dtype or torch.float32
    code = _packed_out_code(dtype)
    count, rows, cols = int(count), int(rows), int(cols)
    th, tw = tiles_hw(cols, rows)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    ptr = _arena(data, count, th * tw, "data")
    fn = _entry("mtq_unpack_tiles_transposed_batched")
    if out is None:
        require_gpu()
        out = torch.empty((count, rows, cols), dtype=dtype, device=data.device)
    elif out.dtype != dtype or out.dim() != 3 or tuple(out.shape) != (count, rows, cols) or out.stride(2) != 1 or not out.is_cuda:
        raise MtqError(f"out must be a {dtype} ({count}, {rows}, {cols}) device tensor with contiguous rows")
    _code, _count, stride, _rows, _cols, ldy = _matrix(out, (3,))
    check(fn(ptr, data.numel(), pm, po, pb, count, rows, cols, out.data_ptr(), code, ldy, stride, _packed_stream_ptr(stream)))
    return out


def packed_matmul(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, stream="current"):
    """mtq_packed_matmul on the current stream: Y = X·P̂ + b for an (m, k) bf16 device tensor X with contiguous rows and the packed
    (k, n) matrix → (m, n) float32 or bfloat16 device tensor.  m = 0 gives the empty (0, n) tensor without a launch."""
    return _packed_product_call("mtq_packed_matmul", True, "m", x, data, tables, n, bias, out_dtype, out, stream)


def packed_matmul_wide(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, stream="current"):
    """mtq_packed_matmul_wide on the current stream: packed_matmul's product, arguments and bits from the wide-block kernel (a
    128 x 128 block whose waves decode whole tiles of the (k, n) stream), for m above the decode range.  Correct for any m; m = 0 gives
    the empty (0, n) tensor without a call."""
    return _packed_product_call("mtq_packed_matmul_wide", True, "m", x, data, tables, n, bias, out_dtype, out, stream)


def has_packed_matmul_wide() -> bool:
    """Whether this build of the library has mtq_packed_matmul_wide (an optional symbol: an older build of the same version lacks it)."""
    return _has(("mtq_packed_matmul_wide",))


PACKED_SKINNY_MAX_M = 32   # include/mtq.h MTQ_PACKED_SKINNY_MAX_M


def packed_linear_skinny_workspace_bytes(m: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_linear_skinny_workspace_bytes (a host function: no GPU): the bytes of workspace the skinny kernel needs for
    (m, n, k, split); split 0 is the library's choice; 0 when the effective split is 1."""
    return _workspace_size("mtq_packed_linear_skinny_workspace_bytes", m, n, k, split)


def packed_linear_skinny(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, split: int = 0, workspace=None,
                         stream="current"):
    """mtq_packed_linear_skinny on the current stream: packed_linear for m <= 32 with a split over K (split 0: the library's choice).
    workspace: a uint8 device tensor of at least packed_linear_skinny_workspace_bytes(m, n, k, split) bytes, 16-byte aligned;
    allocated here when none is given.  The same inputs and the same split give the same bits."""
    return _packed_product_call("mtq_packed_linear_skinny", False, "", x, data, tables, n, bias, out_dtype, out, stream,
                                packed_linear_skinny_workspace_bytes, split, workspace, size_first=True)


PACKED_MATMUL_SKINNY = ("mtq_packed_matmul_skinny_workspace_bytes", "mtq_packed_matmul_skinny")


def has_packed_matmul_skinny() -> bool:
    """Whether this build of the library has mtq_packed_matmul_skinny and its size function (optional symbols: an older build of the
    same version lacks them)."""
    return _has(PACKED_MATMUL_SKINNY)


def packed_matmul_skinny_workspace_bytes(m: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_matmul_skinny_workspace_bytes (a host function: no GPU): the bytes of workspace the skinny (k, n) product needs for
    (m, n, k, split) - n outputs, k contraction; split 0 is the library's choice; 0 when the effective split is 1.  Equal to
    packed_linear_skinny_workspace_bytes for the same arguments."""
    return _workspace_size("mtq_packed_matmul_skinny_workspace_bytes", m, n, k, split)


def packed_matmul_skinny(x, data, tables: PackedTables, n: int, bias=None, out_dtype=None, out=None, split: int = 0, workspace=None,
                         stream="current"):
    """mtq_packed_matmul_skinny on the current stream: packed_matmul for m <= 32 with a split over K (split 0: the library's choice).
    workspace: a uint8 device tensor of at least packed_matmul_skinny_workspace_bytes(m, n, k, split) bytes, 16-byte aligned; allocated
    here when none is given.  Bit for bit packed_linear_skinny at the same split on the all-bf16 packing of the unpacked matrix's
    transpose.  m = 0 gives the empty (0, n) tensor without a launch."""
    return _packed_product_call("mtq_packed_matmul_skinny", True, "m", x, data, tables, n, bias, out_dtype, out, stream,
                                packed_matmul_skinny_workspace_bytes, split, workspace)


def packed_linear_skinny_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_linear_skinny_grouped_workspace_bytes (a host function: no GPU): the bytes of workspace the grouped skinny kernel needs
    for `count` (n, k) experts over total_rows rows; split 0 is the library's choice; 0 when the effective split is 1."""
    return _workspace_size("mtq_packed_linear_skinny_grouped_workspace_bytes", total_rows, count, n, k, split)


def packed_linear_skinny_grouped(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None, out=None,
                                 split: int = 0, workspace=None, stream="current"):
    """mtq_packed_linear_skinny_grouped on the current stream: Y[rows of group e] = X[rows of group e]·Ŵ[e]ᵀ (+ bias[e]) for the `count`
    packed (n, k) experts of one arena (pack_tiles_batched's tables) in one launch.  x: (T, k) bf16 with contiguous rows; group_rows: a
    contiguous int32 device tensor of count + 1 entries, group e owning rows [group_rows[e], group_rows[e + 1]) (the kernel clamps them
    into [0, T]); bias: None or a float32 (count, n) device tensor with contiguous rows.  → (T, n); an `out` allocated here starts as
    zeros, so rows outside every group are zeros.  workspace: as packed_linear_skinny, of
    packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, split) bytes."""
    return _packed_linear_grouped_call("mtq_packed_linear_skinny_grouped", packed_linear_skinny_grouped_workspace_bytes, x, group_rows, arena,
                                       maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, split, workspace, stream)


def _packed_linear_grouped_call(name, workspace_bytes, x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out,
                                split, workspace, stream):
    """The checks and the call the grouped entries share; `workspace_bytes` is the entry's own size function.  split None: an entry
    without a split parameter (the wide one), whose size function takes (T, count, n, k)."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code = _packed_out_code(out_dtype)
    count, n = int(count), int(n)
    x_code, _count, _stride, T, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    if count <= 0 or n <= 0:
        raise MtqError("count and n must be positive")
    th, tw = tiles_hw(n, k)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    ptr = _arena(arena, count, th * tw, "arena")
    pg = _buffer(group_rows, torch.int32, count + 1, "group_rows")
    if group_rows.numel() != count + 1:
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got {group_rows.numel()}")
    bias_ptr, ldb = None, 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.dim() != 2 or tuple(bias.shape) != (count, n) or bias.stride(1) != 1 or not bias.is_cuda:
            raise MtqError(f"bias must be a float32 ({count}, {n}) device tensor with contiguous rows")
        bias_ptr, ldb = bias.data_ptr(), bias.stride(0) if count > 1 else max(bias.stride(0), n)
    need = workspace_bytes(T, count, n, k) if split is None else workspace_bytes(T, count, n, k, split)
    fn = _entry(name)
    out, ldy = _packed_out(out, T, n, out_dtype, x.device, zeros=True)
    ws_ptr, ws_bytes = _packed_workspace(workspace, need, x.device) if need else (None, 0)
    check(fn(x.data_ptr(), T, k, ldx, pg, ptr, arena.numel(), pm, po, pb, count, n, bias_ptr, ldb, out.data_ptr(), code, ldy,
             *(() if split is None else (int(split),)), ws_ptr, ws_bytes, _packed_stream_ptr(stream)))
    return out


def has_packed_linear_grouped_chunked() -> bool:
    """Whether this build of the library has mtq_packed_linear_skinny_grouped_chunked and its size function (optional symbols: an older
    build of the same version lacks them)."""
    return _has(("mtq_packed_linear_skinny_grouped_chunked", "mtq_packed_linear_skinny_grouped_chunked_workspace_bytes"))


def packed_linear_skinny_grouped_chunked_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_linear_skinny_grouped_chunked_workspace_bytes (a host function: no GPU): packed_linear_skinny_grouped_workspace_bytes
    for the same arguments plus the chunk plan's (count + 1) * 4 bytes rounded up to 16.  Never 0."""
    return _workspace_size("mtq_packed_linear_skinny_grouped_chunked_workspace_bytes", total_rows, count, n, k, split)


def packed_linear_skinny_grouped_chunked(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None,
                                         out=None, split: int = 0, workspace=None, stream="current"):
    """mtq_packed_linear_skinny_grouped_chunked on the current stream: packed_linear_skinny_grouped's product, arguments and bits with a
    wave per 32-row chunk of a group (the chunk list is made from group_rows on the device, nothing is read back), for routings with
    hot experts.  workspace: of packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, split) bytes, needed at every
    split; allocated here when none is given."""
    return _packed_linear_grouped_call("mtq_packed_linear_skinny_grouped_chunked", packed_linear_skinny_grouped_chunked_workspace_bytes, x,
                                       group_rows, arena, maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, split, workspace, stream)


WIDE_GROUPED = ("mtq_packed_linear_wide_grouped", "mtq_packed_linear_wide_grouped_workspace_bytes")


def has_packed_linear_wide_grouped() -> bool:
    """Whether this build of the library has mtq_packed_linear_wide_grouped and its size function (optional symbols: an older build of
    the same version lacks them)."""
    return _has(WIDE_GROUPED)


def packed_linear_wide_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int) -> int:
    """mtq_packed_linear_wide_grouped_workspace_bytes (a host function: no GPU): the block plan's (count + 1) * 4 bytes rounded up to
    16, whatever (total_rows, n, k) is.  Never 0."""
    return _workspace_size("mtq_packed_linear_wide_grouped_workspace_bytes", total_rows, count, n, k)


def packed_linear_wide_grouped(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None, out=None,
                               workspace=None, stream="current"):
    """mtq_packed_linear_wide_grouped on the current stream: packed_linear_skinny_grouped's product and arguments (no split) from the
    wide-block kernel, a workgroup per 128 rows x 128 columns of one group (the block list is made from group_rows on the device,
    nothing is read back), for experts with hundreds of rows.  Per group the bits of packed_linear / packed_linear_wide on the group's
    rows, not the skinny family's.  workspace: of packed_linear_wide_grouped_workspace_bytes(T, count, n, k) bytes; allocated here when
    none is given."""
    return _packed_linear_grouped_call("mtq_packed_linear_wide_grouped", packed_linear_wide_grouped_workspace_bytes, x, group_rows, arena,
                                       maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, None, workspace, stream)


MATMUL_GROUPED = ("mtq_packed_matmul_skinny_grouped", "mtq_packed_matmul_skinny_grouped_workspace_bytes")
MATMUL_GROUPED_CHUNKED = ("mtq_packed_matmul_skinny_grouped_chunked", "mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes")
MATMUL_WIDE_GROUPED = ("mtq_packed_matmul_wide_grouped", "mtq_packed_matmul_wide_grouped_workspace_bytes")


def has_packed_matmul_grouped() -> bool:
    """Whether this build of the library has mtq_packed_matmul_skinny_grouped and its size function (optional symbols: an older build of
    the same version lacks them)."""
    return _has(MATMUL_GROUPED)


def has_packed_matmul_grouped_chunked() -> bool:
    """The same for mtq_packed_matmul_skinny_grouped_chunked and its size function."""
    return _has(MATMUL_GROUPED_CHUNKED)


def has_packed_matmul_wide_grouped() -> bool:
    """The same for mtq_packed_matmul_wide_grouped and its size function."""
    return _has(MATMUL_WIDE_GROUPED)


def packed_matmul_skinny_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_matmul_skinny_grouped_workspace_bytes (a host function: no GPU): packed_linear_skinny_grouped_workspace_bytes' answer
    for the same arguments, n the output width and k the contraction of the `count` (k, n) experts."""
    return _workspace_size("mtq_packed_matmul_skinny_grouped_workspace_bytes", total_rows, count, n, k, split)


def packed_matmul_skinny_grouped(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None, out=None,
                                 split: int = 0, workspace=None, stream="current"):
    """mtq_packed_matmul_skinny_grouped on the current stream: Y[rows of group e] = X[rows of group e]·P̂[e] (+ bias[e]) for the `count`
    packed (k, n) experts of one arena (pack_tiles_transposed_batched's or pack_tiles_batched's tables) in one launch.  The arguments
    are packed_linear_skinny_grouped's: x (T, k) bf16 with contiguous rows, group_rows a contiguous int32 device tensor of count + 1
    entries, bias None or float32 (count, n).  → (T, n); an `out` allocated here starts as zeros.  Per 32-row chunk of a group the bits
    of packed_matmul_skinny with that expert's stream and tables at the same split."""
    return _packed_linear_grouped_call("mtq_packed_matmul_skinny_grouped", packed_matmul_skinny_grouped_workspace_bytes, x, group_rows, arena,
                                       maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, split, workspace, stream)


def packed_matmul_skinny_grouped_chunked_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes (a host function: no GPU):
    packed_linear_skinny_grouped_chunked_workspace_bytes' answer for the same arguments.  Never 0."""
    return _workspace_size("mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes", total_rows, count, n, k, split)


def packed_matmul_skinny_grouped_chunked(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None,
                                         out=None, split: int = 0, workspace=None, stream="current"):
    """mtq_packed_matmul_skinny_grouped_chunked on the current stream: packed_matmul_skinny_grouped's product, arguments and bits with a
    wave per 32-row chunk of a group (the chunk list is made from group_rows on the device), for routings with hot experts.  The
    workspace is needed at every split; allocated here when none is given."""
    return _packed_linear_grouped_call("mtq_packed_matmul_skinny_grouped_chunked", packed_matmul_skinny_grouped_chunked_workspace_bytes, x,
                                       group_rows, arena, maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, split, workspace, stream)


def packed_matmul_wide_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int) -> int:
    """mtq_packed_matmul_wide_grouped_workspace_bytes (a host function: no GPU): the block plan's bytes, a function of count.  Never 0."""
    return _workspace_size("mtq_packed_matmul_wide_grouped_workspace_bytes", total_rows, count, n, k)


def packed_matmul_wide_grouped(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, bias=None, out_dtype=None, out=None,
                               workspace=None, stream="current"):
    """mtq_packed_matmul_wide_grouped on the current stream: packed_matmul_skinny_grouped's product and arguments (no split) from the
    wide-block kernel, a workgroup per 128 rows x 128 columns of one group, for experts with hundreds of rows.  Per group the bits of
    packed_matmul / packed_matmul_wide on the group's rows, not the skinny family's."""
    return _packed_linear_grouped_call("mtq_packed_matmul_wide_grouped", packed_matmul_wide_grouped_workspace_bytes, x, group_rows, arena,
                                       maps_dev, offsets_dev, bases_dev, count, n, bias, out_dtype, out, None, workspace, stream)


ACT_CODE = {"silu": 0, "none": 1}   # include/mtq.h MTQ_ACT_SILU, MTQ_ACT_NONE
PACKED_GLU = ("mtq_glu_combine", "mtq_packed_glu_wide", "mtq_packed_glu_wide_grouped", "mtq_packed_glu_wide_grouped_workspace_bytes")


def has_packed_glu() -> bool:
    """Whether this build of the library has the gated entries (mtq_glu_combine, mtq_packed_glu_wide, mtq_packed_glu_wide_grouped and
    its size function; optional symbols: an older build of the same version lacks them)."""
    return _has(PACKED_GLU)


def _act_code(act) -> int:
    if act not in ACT_CODE:
        raise MtqError(f"act must be one of {tuple(ACT_CODE)}, got {act!r}")
    return ACT_CODE[act]


def glu_combine(g, u, act="silu", out_dtype=None, out=None, stream="current"):
    """mtq_glu_combine on the current stream: y = act(g) * u element by element for two float32 (rows, cols) device tensors with
    contiguous rows (any row pitch) → float32 or bfloat16 (rows, cols); the activation is the fused kernels' own function, every
    operation a float32 one.  An empty operand gives the empty result without a call."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code, a = _packed_out_code(out_dtype), _act_code(act)
    for name, t in (("g", g), ("u", u)):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
            raise MtqError(f"{name} must be a float32 2-D device tensor with contiguous rows")
    if tuple(g.shape) != tuple(u.shape):
        raise MtqError(f"g and u must have one shape, got {tuple(g.shape)} and {tuple(u.shape)}")
    rows, cols = (int(v) for v in g.shape)
    fn = _entry("mtq_glu_combine")
    out, ldy = _packed_out(out, rows, cols, out_dtype, g.device)
    if rows == 0 or cols == 0:
        return out
    ldg, ldu = (t.stride(0) if rows > 1 else max(t.stride(0), cols) for t in (g, u))
    check(fn(g.data_ptr(), ldg, u.data_ptr(), ldu, rows, cols, a, out.data_ptr(), code, ldy, _packed_stream_ptr(stream)))
    return out


def _packed_glu_call(name, kn, x, gate_data, gate_tables, up_data, up_tables, n, act, bias_gate, bias_up, out_dtype, out, stream, size=None, split=0,
                     workspace=None):
    """The checks and the call the single-tensor gated entries share; m = 0 or n = 0 ends here with the empty `out`.  size: a skinny
    entry's own size function, which makes the call one with m <= 32, a split and a workspace (never of 0 bytes)."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code, a = _packed_out_code(out_dtype), _act_code(act)
    x_code, _count, _stride, m, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    if size is not None and m > PACKED_SKINNY_MAX_M:
        raise MtqError(f"the skinny kernel takes m <= {PACKED_SKINNY_MAX_M}, got m = {m}")
    grid = tiles_hw(k, n) if kn else tiles_hw(n, k)
    for side, tables in (("gate ", gate_tables), ("up ", up_tables)):
        if grid != (tables.tiles_h, tables.tiles_w):
            raise _grid_error(tables, n, k, kn, side)
    pg, pu = _packed_stream(gate_data, gate_tables, "gate data"), _packed_stream(up_data, up_tables, "up data")
    bg = None if bias_gate is None else _buffer(bias_gate, torch.float32, n, "bias_gate")
    bu = None if bias_up is None else _buffer(bias_up, torch.float32, n, "bias_up")
    fn = _entry(name)
    out, ldy = _packed_out(out, m, n, out_dtype, x.device)
    if m == 0 or n == 0:                             # the entry refuses empty operands: they end here
        return out
    more = () if size is None else (int(split), *_packed_workspace(workspace, size(m, n, k, split), x.device))
    check(fn(x.data_ptr(), m, k, ldx, pg, gate_tables.nbytes, gate_tables.map_ptr, gate_tables.offsets_ptr, pu, up_tables.nbytes,
             up_tables.map_ptr, up_tables.offsets_ptr, n, bg, bu, a, out.data_ptr(), code, ldy, *more, _packed_stream_ptr(stream)))
    return out


def packed_glu_wide(x, gate_data, gate_tables: PackedTables, up_data, up_tables: PackedTables, n: int, act="silu", bias_gate=None, bias_up=None,
                    out_dtype=None, out=None, stream="current"):
    """mtq_packed_glu_wide on the current stream: act(X·Ŵgᵀ + bg) * (X·Ŵuᵀ + bu) for an (m, k) bf16 device tensor X and two packed
    (n, k) weights in one launch → (m, n) float32 or bfloat16: bit for bit two packed_linear calls into float32 and glu_combine.
    m = 0 or n = 0 gives the empty (m, n) tensor without a launch."""
    return _packed_glu_call("mtq_packed_glu_wide", False, x, gate_data, gate_tables, up_data, up_tables, n, act, bias_gate, bias_up, out_dtype, out, stream)


def packed_glu_wide_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int) -> int:
    """mtq_packed_glu_wide_grouped_workspace_bytes (a host function: no GPU): packed_linear_wide_grouped_workspace_bytes' answer."""
    return _workspace_size("mtq_packed_glu_wide_grouped_workspace_bytes", total_rows, count, n, k)


def _packed_glu_grouped_call(name, workspace_bytes, x, group_rows, gate, up, count, n, act, bias_gate, bias_up, out_dtype, out, split, workspace,
                             stream, size_first=False):
    """The checks and the call the grouped gated entries of both orientations share (the grid of `count` (n, k) weights has as many tiles
    as that of (k, n) matrices); `workspace_bytes` is the entry's own size function.  split None: an entry without a split parameter (a
    wide one), whose size function takes (T, count, n, k).  size_first: the size is asked before the entry is looked up."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code, a = _packed_out_code(out_dtype), _act_code(act)
    count, n = int(count), int(n)
    x_code, _count, _stride, T, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    if count <= 0 or n <= 0:
        raise MtqError("count and n must be positive")
    th, tw = tiles_hw(n, k)
    sides = []
    for which, (arena, maps_dev, offsets_dev, bases_dev) in (("gate", gate), ("up", up)):
        pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
        sides += [_arena(arena, count, th * tw, f"the {which} arena"), arena.numel(), pm, po, pb]
    pg = _buffer(group_rows, torch.int32, count + 1, "group_rows")
    if group_rows.numel() != count + 1:
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got {group_rows.numel()}")
    ptrs, ldb = [], 0
    for which, bias in (("bias_gate", bias_gate), ("bias_up", bias_up)):
        if bias is None:
            ptrs.append(None)
            continue
        if bias.dtype != torch.float32 or bias.dim() != 2 or tuple(bias.shape) != (count, n) or bias.stride(1) != 1 or not bias.is_cuda:
            raise MtqError(f"{which} must be a float32 ({count}, {n}) device tensor with contiguous rows")
        pitch = bias.stride(0) if count > 1 else max(bias.stride(0), n)
        if ldb and pitch != ldb:
            raise MtqError("bias_gate and bias_up must have one row pitch")
        ptrs.append(bias.data_ptr())
        ldb = pitch
    more = () if split is None else (int(split),)
    need = workspace_bytes(T, count, n, k, *more) if size_first and T else None
    fn = _entry(name)
    out, ldy = _packed_out(out, T, n, out_dtype, x.device, zeros=True)
    if T == 0:
        return out
    ws_ptr, ws_bytes = _packed_workspace(workspace, workspace_bytes(T, count, n, k, *more) if need is None else need, x.device)
    check(fn(x.data_ptr(), T, k, ldx, pg, *sides, count, n, ptrs[0], ptrs[1], ldb, a, out.data_ptr(), code, ldy, *more, ws_ptr, ws_bytes,
             _packed_stream_ptr(stream)))
    return out


def packed_glu_wide_grouped(x, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None, out=None,
                            workspace=None, stream="current"):
    """mtq_packed_glu_wide_grouped on the current stream: packed_glu_wide's product for the `count` experts of two arenas, each over its
    own rows of X, in one launch.  gate, up: (arena, maps_dev, offsets_dev, bases_dev) as packed_linear_wide_grouped takes them, of
    `count` (n, k) experts each; x, group_rows, out and workspace as there; bias_gate, bias_up: None or float32 (count, n) device
    tensors of one row pitch.  Per group the bits of two packed_linear calls into float32 and glu_combine on the group's rows.  An
    `out` allocated here starts as zeros, so rows outside every group are zeros."""
    return _packed_glu_grouped_call("mtq_packed_glu_wide_grouped", packed_glu_wide_grouped_workspace_bytes, x, group_rows, gate, up, count, n, act,
                                    bias_gate, bias_up, out_dtype, out, None, workspace, stream, size_first=True)


PACKED_GLU_SKINNY = ("mtq_packed_glu_skinny_workspace_bytes", "mtq_packed_glu_skinny", "mtq_packed_glu_skinny_grouped_workspace_bytes",
                     "mtq_packed_glu_skinny_grouped")


def has_packed_glu_skinny() -> bool:
    """Whether this build of the library has the fused gated entries for decode (mtq_packed_glu_skinny, mtq_packed_glu_skinny_grouped and
    their size functions; optional symbols: an older build of the same version lacks them)."""
    return _has(PACKED_GLU_SKINNY)


def packed_glu_skinny_workspace_bytes(m: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_glu_skinny_workspace_bytes (a host function: no GPU): the bytes of workspace the fused decode call needs for
    (m, n, k, split); split 0 is the library's choice.  Never 0: both projections' partial sums go through it at every split."""
    return _workspace_size("mtq_packed_glu_skinny_workspace_bytes", m, n, k, split)


def packed_glu_skinny(x, gate_data, gate_tables: PackedTables, up_data, up_tables: PackedTables, n: int, act="silu", bias_gate=None,
                      bias_up=None, out_dtype=None, out=None, split: int = 0, workspace=None, stream="current"):
    """mtq_packed_glu_skinny on the current stream: packed_glu_wide's product for m <= 32 with a split over K (split 0: the library's
    choice), two launches: bit for bit two packed_linear_skinny calls into float32 at that split and glu_combine.  workspace: a uint8
    device tensor of at least packed_glu_skinny_workspace_bytes(m, n, k, split) bytes, 16-byte aligned; allocated here when none is
    given.  m = 0 or n = 0 gives the empty (m, n) tensor without a launch."""
    return _packed_glu_call("mtq_packed_glu_skinny", False, x, gate_data, gate_tables, up_data, up_tables, n, act, bias_gate, bias_up, out_dtype, out,
                            stream, packed_glu_skinny_workspace_bytes, split, workspace)


def packed_glu_skinny_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_glu_skinny_grouped_workspace_bytes (a host function: no GPU): packed_glu_skinny_workspace_bytes for the grouped call,
    total_rows in place of m and the grouped entry's own split rule at split 0."""
    return _workspace_size("mtq_packed_glu_skinny_grouped_workspace_bytes", total_rows, count, n, k, split)


def packed_glu_skinny_grouped(x, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None, out=None,
                              split: int = 0, workspace=None, stream="current"):
    """mtq_packed_glu_skinny_grouped on the current stream: packed_glu_wide_grouped's operands and product from the skinny family's
    split over K, for decode-sized groups: per group the bits of two packed_linear_skinny_grouped calls into float32 at that split
    and glu_combine.  An `out` allocated here starts as zeros, so rows outside every group are zeros."""
    return _packed_glu_grouped_call("mtq_packed_glu_skinny_grouped", packed_glu_skinny_grouped_workspace_bytes, x, group_rows, gate, up, count, n, act,
                                    bias_gate, bias_up, out_dtype, out, split, workspace, stream)


PACKED_GLU_MATMUL = ("mtq_packed_glu_matmul_wide", "mtq_packed_glu_matmul_wide_grouped", "mtq_packed_glu_matmul_wide_grouped_workspace_bytes")
PACKED_GLU_MATMUL_SKINNY = ("mtq_packed_glu_matmul_skinny_workspace_bytes", "mtq_packed_glu_matmul_skinny",
                            "mtq_packed_glu_matmul_skinny_grouped_workspace_bytes", "mtq_packed_glu_matmul_skinny_grouped")


def has_packed_glu_matmul() -> bool:
    """Whether this build of the library has the gated entries for (k, n) weights (mtq_packed_glu_matmul_wide,
    mtq_packed_glu_matmul_wide_grouped and its size function; optional symbols: an older build of the same version lacks them)."""
    return _has(PACKED_GLU_MATMUL)


def has_packed_glu_matmul_skinny() -> bool:
    """Whether this build of the library has the fused gated entries for (k, n) weights at decode (mtq_packed_glu_matmul_skinny,
    mtq_packed_glu_matmul_skinny_grouped and their size functions; optional symbols)."""
    return _has(PACKED_GLU_MATMUL_SKINNY)


def packed_glu_matmul_wide(x, gate_data, gate_tables: PackedTables, up_data, up_tables: PackedTables, n: int, act="silu", bias_gate=None,
                           bias_up=None, out_dtype=None, out=None, stream="current"):
    """mtq_packed_glu_matmul_wide on the current stream: act(X·P̂g + bg) * (X·P̂u + bu) for an (m, k) bf16 device tensor X and two packed
    (k, n) matrices in one launch → (m, n) float32 or bfloat16: bit for bit two packed_matmul calls into float32 and glu_combine.
    m = 0 or n = 0 gives the empty (m, n) tensor without a launch."""
    return _packed_glu_call("mtq_packed_glu_matmul_wide", True, x, gate_data, gate_tables, up_data, up_tables, n, act, bias_gate, bias_up, out_dtype, out, stream)


def packed_glu_matmul_wide_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int) -> int:
    """mtq_packed_glu_matmul_wide_grouped_workspace_bytes (a host function: no GPU): packed_glu_wide_grouped_workspace_bytes' answer."""
    return _workspace_size("mtq_packed_glu_matmul_wide_grouped_workspace_bytes", total_rows, count, n, k)


def packed_glu_matmul_wide_grouped(x, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None,
                                   out=None, workspace=None, stream="current"):
    """mtq_packed_glu_matmul_wide_grouped on the current stream: packed_glu_matmul_wide's product for the `count` (k, n) experts of two
    arenas, each over its own rows of X, in one launch.  Operands as packed_glu_wide_grouped takes them.  Per group the bits of two
    packed_matmul calls into float32 and glu_combine on the group's rows.  An `out` allocated here starts as zeros."""
    return _packed_glu_grouped_call("mtq_packed_glu_matmul_wide_grouped", packed_glu_matmul_wide_grouped_workspace_bytes, x, group_rows, gate, up, count, n, act,
                                    bias_gate, bias_up, out_dtype, out, None, workspace, stream)


def packed_glu_matmul_skinny_workspace_bytes(m: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_glu_matmul_skinny_workspace_bytes (a host function: no GPU): packed_glu_skinny_workspace_bytes' answer."""
    return _workspace_size("mtq_packed_glu_matmul_skinny_workspace_bytes", m, n, k, split)


def packed_glu_matmul_skinny(x, gate_data, gate_tables: PackedTables, up_data, up_tables: PackedTables, n: int, act="silu", bias_gate=None,
                             bias_up=None, out_dtype=None, out=None, split: int = 0, workspace=None, stream="current"):
    """mtq_packed_glu_matmul_skinny on the current stream: packed_glu_matmul_wide's product for m <= 32 with a split over K (split 0: the
    library's choice), two launches: bit for bit two packed_matmul_skinny calls into float32 at that split and glu_combine.  workspace
    as packed_glu_skinny takes it.  m = 0 or n = 0 gives the empty (m, n) tensor without a launch."""
    return _packed_glu_call("mtq_packed_glu_matmul_skinny", True, x, gate_data, gate_tables, up_data, up_tables, n, act, bias_gate, bias_up, out_dtype,
                            out, stream, packed_glu_matmul_skinny_workspace_bytes, split, workspace)


def packed_glu_matmul_skinny_grouped_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0) -> int:
    """mtq_packed_glu_matmul_skinny_grouped_workspace_bytes (a host function: no GPU): packed_glu_skinny_grouped_workspace_bytes' answer."""
    return _workspace_size("mtq_packed_glu_matmul_skinny_grouped_workspace_bytes", total_rows, count, n, k, split)


def packed_glu_matmul_skinny_grouped(x, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None,
                                     out=None, split: int = 0, workspace=None, stream="current"):
    """mtq_packed_glu_matmul_skinny_grouped on the current stream: packed_glu_matmul_wide_grouped's operands and product from the skinny
    family's split over K, for decode-sized groups: per group the bits of two packed_matmul_skinny_grouped calls into float32 at that
    split and glu_combine.  An `out` allocated here starts as zeros, so rows outside every group are zeros."""
    return _packed_glu_grouped_call("mtq_packed_glu_matmul_skinny_grouped", packed_glu_matmul_skinny_grouped_workspace_bytes, x, group_rows, gate, up, count, n, act,
                                    bias_gate, bias_up, out_dtype, out, split, workspace, stream)


# ---- the grouped skinny GLU with a wave per 32-row chunk (include/mtq_glu_chunked.h): [kn] → (entry, size function)
PACKED_GLU_SKINNY_GROUPED_CHUNKED = (
    ("mtq_packed_glu_skinny_grouped_chunked", "mtq_packed_glu_skinny_grouped_chunked_workspace_bytes"),
    ("mtq_packed_glu_matmul_skinny_grouped_chunked", "mtq_packed_glu_matmul_skinny_grouped_chunked_workspace_bytes"))


def glu_grouped_chunked_bound(kn: bool = False) -> bool:
    """Whether this build of the library has mtq_packed_glu_skinny_grouped_chunked and its size function, or with `kn` the matmul twin's
    pair (optional symbols: an older build of the same version lacks them)."""
    return _has(PACKED_GLU_SKINNY_GROUPED_CHUNKED[bool(kn)])


def glu_grouped_chunked_workspace_bytes(total_rows: int, count: int, n: int, k: int, split: int = 0, kn: bool = False) -> int:
    """mtq_packed_glu_skinny_grouped_chunked_workspace_bytes (kn: its matmul twin; host functions: no GPU): the plan region,
    (count + 1) * 4 bytes rounded up to 16, and behind it packed_glu_skinny_grouped_workspace_bytes' answer."""
    return _workspace_size(PACKED_GLU_SKINNY_GROUPED_CHUNKED[bool(kn)][1], total_rows, count, n, k, split)


def glu_grouped_chunked(x, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None, out=None,
                        split: int = 0, workspace=None, kn: bool = False, stream="current"):
    """mtq_packed_glu_skinny_grouped_chunked (kn: its matmul twin) on the current stream: packed_glu_skinny_grouped's
    (packed_glu_matmul_skinny_grouped's) operands and, for a nondecreasing group_rows, its bits at the same split, with a wave per 32-row
    chunk of a group (the chunks are planned on the device: nothing is read back), for routings with experts of many rows.  workspace: an
    optional uint8 device tensor of glu_grouped_chunked_workspace_bytes bytes."""
    name = PACKED_GLU_SKINNY_GROUPED_CHUNKED[bool(kn)][0]

    def size(*args):
        return glu_grouped_chunked_workspace_bytes(*args, kn=kn)

    return _packed_glu_grouped_call(name, size, x, group_rows, gate, up, count, n, act, bias_gate, bias_up, out_dtype, out, split, workspace, stream)


MOE = ("mtq_moe_plan_workspace_bytes", "mtq_moe_plan", "mtq_moe_dispatch", "mtq_moe_combine")
MOE_MAX_TOPK, MOE_MAX_EXPERTS, MOE_RUN = 64, 4096, 1024   # include/mtq.h MTQ_MOE_MAX_TOPK, MTQ_MOE_MAX_EXPERTS, MTQ_MOE_RUN
IDS_I32, IDS_I64 = 0, 1                                   # include/mtq.h MTQ_IDS_I32, MTQ_IDS_I64


def has_moe() -> bool:
    """Whether this build of the library has the MoE routing entries (mtq_moe_plan and its size function, mtq_moe_dispatch,
    mtq_moe_combine; optional symbols: an older build of the same version lacks them)."""
    return _has(MOE)


def moe_plan_workspace_bytes(tokens: int, topk: int, count: int) -> int:
    """mtq_moe_plan_workspace_bytes (a host function: no GPU): ceil(tokens * topk / MOE_RUN) * count * 4 rounded up to 16.  Never 0."""
    return _workspace_size("mtq_moe_plan_workspace_bytes", tokens, topk, count)


def _rows_ld(t, rows: int, cols: int) -> int:
    """The row pitch of a 2-D tensor with contiguous rows, as the entries' pitch checks expect it of a single row."""
    return t.stride(0) if rows > 1 else max(t.stride(0), cols)


def moe_plan(topk_ids, count: int, workspace=None, stream="current"):
    """mtq_moe_plan on the current stream: topk_ids, a (tokens, topk) int32 or int64 device tensor with contiguous rows (any row
    pitch; read in its own width), → (group_rows int32 [count + 1], row_of int32 [S], src int32 [S]), S = tokens * topk: the stable
    counting sort of the slots by expert, ids outside [0, count) dropped (row_of -1; src[R:] is -1).  One launch up to S = MOE_RUN,
    three above; nothing is read back.  workspace: a uint8 device tensor of at least moe_plan_workspace_bytes(tokens, topk, count)
    bytes, 16-byte aligned; allocated here when none is given."""
    torch = _torch()
    if topk_ids.dim() != 2:
        raise MtqError(f"topk_ids must be a 2-D (tokens, topk) tensor, got {topk_ids.dim()}-D")
    if topk_ids.dtype not in (torch.int32, torch.int64):
        raise MtqError(f"topk_ids must be int32 or int64, got {topk_ids.dtype}")
    T, K = (int(v) for v in topk_ids.shape)
    if K > 1 and topk_ids.stride(1) != 1:
        raise MtqError("topk_ids must have contiguous rows (stride(1) == 1)")
    if not topk_ids.is_cuda:
        raise MtqError("expected a device tensor (the hip backend has no CPU fallback)")
    need = moe_plan_workspace_bytes(T, K, count)      # the limits on tokens, topk and count are the library's
    fn = _entry("mtq_moe_plan")
    if workspace is not None:
        ws_ptr, ws_bytes = _packed_workspace(workspace, need, topk_ids.device)
    require_gpu()
    group_rows = torch.empty((int(count) + 1,), dtype=torch.int32, device=topk_ids.device)
    row_of, src = (torch.empty((T * K,), dtype=torch.int32, device=topk_ids.device) for _ in range(2))
    if workspace is None:       # after the outputs: a workspace made here is the allocator's again once its pointer is taken, and must not
        ws_ptr, ws_bytes = _packed_workspace(None, need, topk_ids.device)       # become one of them (the three-kernel plan reads it back)
    check(fn(topk_ids.data_ptr(), IDS_I64 if topk_ids.dtype == torch.int64 else IDS_I32, _rows_ld(topk_ids, T, K), T, K, int(count),
             group_rows.data_ptr(), row_of.data_ptr(), src.data_ptr(), ws_ptr, ws_bytes, _packed_stream_ptr(stream)))
    return group_rows, row_of, src


def moe_dispatch(x, src, topk: int, out=None, stream="current"):
    """mtq_moe_dispatch on the current stream: xs[r] = x[src[r] // topk] for x (tokens, k) bf16 with contiguous rows and src, a
    contiguous int32 device tensor of S = tokens * topk entries, → xs (S, k) bf16; a row whose src is outside [0, S) is zeros.  Every
    row of xs is written; `out`: a bf16 (S, k) device tensor with contiguous rows (any row pitch)."""
    torch = _torch()
    x_code, _count, _stride, T, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    topk = int(topk)
    S = T * topk
    if T <= 0 or k <= 0 or topk <= 0:
        raise MtqError("tokens, k and topk must be positive")
    ps = _buffer(src, torch.int32, S, "src")
    if src.numel() != S:
        raise MtqError(f"src must have tokens * topk = {S} entries, got {src.numel()}")
    fn = _entry("mtq_moe_dispatch")
    out, ldxs = _packed_out(out, S, k, torch.bfloat16, x.device)
    check(fn(x.data_ptr(), T, k, ldx, ps, topk, out.data_ptr(), ldxs, _packed_stream_ptr(stream)))
    return out


def moe_combine(ys, row_of, weights, base=None, out_dtype=None, out=None, stream="current"):
    """mtq_moe_combine on the current stream: y[t] = base[t] + the sum over j, in that order, of weights[t, j] * ys[row_of[t * topk + j]]
    in separately rounded float32 operations, a slot whose row is outside [0, S) skipped.  ys: (>= S, n) bf16 or float32; row_of: a
    contiguous int32 device tensor of S = tokens * topk entries; weights: (tokens, topk) float32; base: None or (tokens, n) bf16 or
    float32; all device tensors with contiguous rows (any row pitch) → (tokens, n) float32 or bfloat16."""
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code = _packed_out_code(out_dtype)
    if weights.dim() != 2 or weights.dtype != torch.float32 or (weights.shape[1] > 1 and weights.stride(1) != 1) or not weights.is_cuda:
        raise MtqError("weights must be a float32 (tokens, topk) device tensor with contiguous rows")
    T, K = (int(v) for v in weights.shape)
    S = T * K
    if T <= 0 or K <= 0:
        raise MtqError("tokens and topk must be positive")
    ys_code, _count, _stride, rows, n, ldys = _matrix(ys, (2,))
    if rows < S or n <= 0:
        raise MtqError(f"ys must be ({S}, n) or longer, got {tuple(ys.shape)}")
    pr = _buffer(row_of, torch.int32, S, "row_of")
    if row_of.numel() != S:
        raise MtqError(f"row_of must have tokens * topk = {S} entries, got {row_of.numel()}")
    base_ptr, base_code, ldbase = None, 0, 0
    if base is not None:
        base_code, _count, _stride, brows, bcols, ldbase = _matrix(base, (2,))
        if (brows, bcols) != (T, n):
            raise MtqError(f"base must be ({T}, {n}), got {tuple(base.shape)}")
        base_ptr = base.data_ptr()
    fn = _entry("mtq_moe_combine")
    out, ldy = _packed_out(out, T, n, out_dtype, ys.device)
    check(fn(ys.data_ptr(), ys_code, ldys, pr, weights.data_ptr(), _rows_ld(weights, T, K), base_ptr, base_code, ldbase, T, K, n,
             out.data_ptr(), code, ldy, _packed_stream_ptr(stream)))
    return out


# ---- MoE decode without the staging copies (include/mtq_moe_decode.h): [kn] → (entry, size function)
MOE_GATHER = (("mtq_packed_glu_skinny_grouped_gather", "mtq_packed_glu_skinny_grouped_gather_workspace_bytes"),
              ("mtq_packed_glu_matmul_skinny_grouped_gather", "mtq_packed_glu_matmul_skinny_grouped_gather_workspace_bytes"))
MOE_DOWN_COMBINE = (("mtq_packed_linear_skinny_grouped_combine", "mtq_packed_linear_skinny_grouped_combine_workspace_bytes"),
                    ("mtq_packed_matmul_skinny_grouped_combine", "mtq_packed_matmul_skinny_grouped_combine_workspace_bytes"))
# their forms with a wave per 32-row chunk (include/mtq_glu_chunked.h), and kernel → the tables
MOE_GATHER_CHUNKED = (("mtq_packed_glu_skinny_grouped_chunked_gather", "mtq_packed_glu_skinny_grouped_chunked_gather_workspace_bytes"),
                      ("mtq_packed_glu_matmul_skinny_grouped_chunked_gather", "mtq_packed_glu_matmul_skinny_grouped_chunked_gather_workspace_bytes"))
MOE_DOWN_COMBINE_CHUNKED = (
    ("mtq_packed_linear_skinny_grouped_chunked_combine", "mtq_packed_linear_skinny_grouped_chunked_combine_workspace_bytes"),
    ("mtq_packed_matmul_skinny_grouped_chunked_combine", "mtq_packed_matmul_skinny_grouped_chunked_combine_workspace_bytes"))
MOE_DECODE_KERNELS = ("walk", "chunks")
_MOE_GATHER_OF = {"walk": MOE_GATHER, "chunks": MOE_GATHER_CHUNKED}
_MOE_DOWN_COMBINE_OF = {"walk": MOE_DOWN_COMBINE, "chunks": MOE_DOWN_COMBINE_CHUNKED}


def _moe_decode_pair(table, kernel: str, kn: bool):
    if kernel not in MOE_DECODE_KERNELS:
        raise MtqError(f"kernel must be one of {MOE_DECODE_KERNELS}, got {kernel!r}")
    return table[kernel][bool(kn)]


def moe_decode_chunked_bound(kn: bool = False) -> bool:
    """moe_decode_bound for the entries with a wave per 32-row chunk (optional symbols)."""
    return _has(MOE_GATHER_CHUNKED[bool(kn)] + MOE_DOWN_COMBINE_CHUNKED[bool(kn)])


def moe_decode_bound(kn: bool = False) -> bool:
    """Whether this build of the library has the gathered grouped GLU and the down projection with the combine in its reduce for
    (n, k) experts, or with `kn` for (k, n) experts (optional symbols: an older build of the same version lacks them)."""
    return _has(MOE_GATHER[bool(kn)] + MOE_DOWN_COMBINE[bool(kn)])


def moe_glu_gather_workspace_bytes(slots: int, count: int, n: int, k: int, split: int = 0, kn: bool = False, kernel: str = "walk") -> int:
    """The *_gather_workspace_bytes size functions (host functions: no GPU): packed_glu_skinny_grouped_workspace_bytes' answer for
    total_rows = slots = tokens * topk; kernel "chunks": the chunked entry's, the plan region more."""
    return _workspace_size(_moe_decode_pair(_MOE_GATHER_OF, kernel, kn)[1], slots, count, n, k, split)


def moe_down_combine_workspace_bytes(slots: int, count: int, n: int, k: int, split: int = 0, kn: bool = False, kernel: str = "walk") -> int:
    """The *_combine_workspace_bytes size functions (host functions: no GPU): max(effective split, 1) * slots * n * 4 bytes rounded up
    to 16, the effective split packed_linear_skinny_grouped's for (slots, count, n, k, split).  Never 0.  kernel "chunks": the chunked
    entry's, the plan region more."""
    return _workspace_size(_moe_decode_pair(_MOE_DOWN_COMBINE_OF, kernel, kn)[1], slots, count, n, k, split)


def moe_glu_gather(x, src, topk: int, group_rows, gate, up, count: int, n: int, act="silu", bias_gate=None, bias_up=None, out_dtype=None,
                   out=None, split: int = 0, workspace=None, kn: bool = False, stream="current", kernel: str = "walk"):
    """mtq_packed_glu_skinny_grouped_gather (kn: its matmul twin) on the current stream: packed_glu_skinny_grouped on the rows
    moe_dispatch would have written, without writing them.  x: the (tokens, k) bf16 token matrix with contiguous rows; src: the plan's
    contiguous int32 device tensor of S = tokens * topk entries; group_rows, gate, up, the biases, split and workspace as
    packed_glu_skinny_grouped takes them → (S, n); an `out` allocated here starts as zeros, so rows of no group are zeros.
    kernel (MOE_DECODE_KERNELS): "chunks", mtq_packed_glu_skinny_grouped_chunked_gather - the same bits from a wave per 32-row chunk."""
    name, size = _moe_decode_pair(_MOE_GATHER_OF, kernel, kn)
    torch = _torch()
    out_dtype = out_dtype or torch.float32
    code, a = _packed_out_code(out_dtype), _act_code(act)
    count, n, topk = int(count), int(n), int(topk)
    x_code, _count, _stride, T, k, ldx = _matrix(x, (2,))
    if x_code != DTYPE_BF16:
        raise MtqError("x must be a bfloat16 tensor")
    if count <= 0 or n <= 0 or T <= 0 or topk <= 0:
        raise MtqError("tokens, topk, count and n must be positive")
    S = T * topk
    th, tw = tiles_hw(n, k)
    sides = []
    for which, (arena, maps_dev, offsets_dev, bases_dev) in (("gate", gate), ("up", up)):
        pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
        sides += [_arena(arena, count, th * tw, f"the {which} arena"), arena.numel(), pm, po, pb]
    pg = _buffer(group_rows, torch.int32, count + 1, "group_rows")
    if group_rows.numel() != count + 1:
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got {group_rows.numel()}")
    ps = _buffer(src, torch.int32, S, "src")
    if src.numel() != S:
        raise MtqError(f"src must have tokens * topk = {S} entries, got {src.numel()}")
    ptrs, ldb = [], 0
    for which, bias in (("bias_gate", bias_gate), ("bias_up", bias_up)):
        if bias is None:
            ptrs.append(None)
            continue
        if bias.dtype != torch.float32 or bias.dim() != 2 or tuple(bias.shape) != (count, n) or bias.stride(1) != 1 or not bias.is_cuda:
            raise MtqError(f"{which} must be a float32 ({count}, {n}) device tensor with contiguous rows")
        pitch = bias.stride(0) if count > 1 else max(bias.stride(0), n)
        if ldb and pitch != ldb:
            raise MtqError("bias_gate and bias_up must have one row pitch")
        ptrs.append(bias.data_ptr())
        ldb = pitch
    fn = _entry(name)
    need = _workspace_size(size, S, count, n, k, split)
    out, ldy = _packed_out(out, S, n, out_dtype, x.device, zeros=True)
    ws_ptr, ws_bytes = _packed_workspace(workspace, need, x.device)
    check(fn(x.data_ptr(), T, topk, k, ldx, ps, pg, *sides, count, n, ptrs[0], ptrs[1], ldb, a, out.data_ptr(), code, ldy, int(split), ws_ptr,
             ws_bytes, _packed_stream_ptr(stream)))
    return out


def moe_down_combine(h, group_rows, arena, maps_dev, offsets_dev, bases_dev, count: int, n: int, row_of, weights, base=None, expert_dtype=None,
                     out_dtype=None, out=None, split: int = 0, workspace=None, kn: bool = False, stream="current", kernel: str = "walk"):
    """mtq_packed_linear_skinny_grouped_combine (kn: its matmul twin) on the current stream: packed_linear_skinny_grouped without bias
    into expert_dtype and moe_combine of its rows, without those rows being written.  h: (S, k) bf16 with contiguous rows,
    S = tokens * topk; group_rows and the arena's tables as packed_linear_skinny_grouped takes them; row_of, weights (tokens, topk)
    float32 and base as moe_combine takes them → (tokens, n) float32 or bfloat16.
    kernel (MOE_DECODE_KERNELS): "chunks", mtq_packed_linear_skinny_grouped_chunked_combine - the same bits from a wave per 32-row chunk."""
    name, size = _moe_decode_pair(_MOE_DOWN_COMBINE_OF, kernel, kn)
    torch = _torch()
    out_dtype, expert_dtype = out_dtype or torch.float32, expert_dtype or torch.float32
    code, expert_code = _packed_out_code(out_dtype), _packed_out_code(expert_dtype)
    count, n = int(count), int(n)
    if weights.dim() != 2 or weights.dtype != torch.float32 or (weights.shape[1] > 1 and weights.stride(1) != 1) or not weights.is_cuda:
        raise MtqError("weights must be a float32 (tokens, topk) device tensor with contiguous rows")
    T, K = (int(v) for v in weights.shape)
    S = T * K
    if T <= 0 or K <= 0 or count <= 0 or n <= 0:
        raise MtqError("tokens, topk, count and n must be positive")
    h_code, _count, _stride, rows, k, ldx = _matrix(h, (2,))
    if h_code != DTYPE_BF16:
        raise MtqError("h must be a bfloat16 tensor")
    if rows != S:
        raise MtqError(f"h must be ({S}, k), one row per slot, got {tuple(h.shape)}")
    th, tw = tiles_hw(n, k)
    pm, po, pb = _batch_tables(maps_dev, offsets_dev, bases_dev, count, th * tw)
    ptr = _arena(arena, count, th * tw, "arena")
    pg = _buffer(group_rows, torch.int32, count + 1, "group_rows")
    if group_rows.numel() != count + 1:
        raise MtqError(f"group_rows must have count + 1 = {count + 1} entries, got {group_rows.numel()}")
    pr = _buffer(row_of, torch.int32, S, "row_of")
    if row_of.numel() != S:
        raise MtqError(f"row_of must have tokens * topk = {S} entries, got {row_of.numel()}")
    base_ptr, base_code, ldbase = None, 0, 0
    if base is not None:
        base_code, _count, _stride, brows, bcols, ldbase = _matrix(base, (2,))
        if (brows, bcols) != (T, n):
            raise MtqError(f"base must be ({T}, {n}), got {tuple(base.shape)}")
        base_ptr = base.data_ptr()
    fn = _entry(name)
    need = _workspace_size(size, S, count, n, k, split)
    out, ldy = _packed_out(out, T, n, out_dtype, h.device)
    ws_ptr, ws_bytes = _packed_workspace(workspace, need, h.device)
    check(fn(h.data_ptr(), k, ldx, pg, ptr, arena.numel(), pm, po, pb, count, n, expert_code, pr, weights.data_ptr(), _rows_ld(weights, T, K),
             base_ptr, base_code, ldbase, T, K, out.data_ptr(), code, ldy, int(split), ws_ptr, ws_bytes, _packed_stream_ptr(stream)))
    return out

MOE_ROUTE = ("mtq_moe_route",)
ROUTE_SOFTMAX, ROUTE_SIGMOID = 0, 1                       # include/mtq.h MTQ_ROUTE_SOFTMAX, MTQ_ROUTE_SIGMOID
MOE_MAX_GROUPS = 64                                       # include/mtq.h MTQ_MOE_MAX_GROUPS
ROUTE_SCORES = {"softmax": ROUTE_SOFTMAX, "sigmoid": ROUTE_SIGMOID}


def _route_out(out, rows: int, cols: int, dtype, device, name: str):
    """An output of moe_route checked, or a new (rows, cols) tensor → (tensor, pitch)."""
    torch = _torch()
    if out is None:
        require_gpu()
        out = torch.empty((rows, cols), dtype=dtype, device=device)
    elif out.dtype != dtype or out.dim() != 2 or tuple(out.shape) != (rows, cols) or (cols > 1 and out.stride(1) != 1) or not out.is_cuda:
        raise MtqError(f"{name} must be a {dtype} ({rows}, {cols}) device tensor with contiguous rows")
    return out, _rows_ld(out, rows, cols)


def moe_route(logits, topk: int, score: str = "softmax", bias=None, n_group: int = 1, topk_group: int = 1, group_top: int = 2,
              renormalize: bool = True, eps: float = 0.0, scale: float = 1.0, return_scores: bool = False, out_ids=None, out_weights=None,
              out_scores=None, stream="current"):
    """mtq_moe_route on the current stream: logits, a (tokens, count) bf16 or float32 device tensor with contiguous rows (any row
    pitch), → (topk_ids int32 (tokens, topk), topk_weights float32 (tokens, topk), scores float32 (tokens, count) or None) in one
    launch: softmax or sigmoid scores, an optional float32 [count] selection bias, group-limited top-k and the weights' renormalising
    and scaling, by the rule include/mtq.h states.  The scores are written when return_scores is set or out_scores is given.
    out_ids, out_weights, out_scores: optional device tensors of those types and shapes with contiguous rows (any row pitch).  The
    limits on count, topk, the groups, eps and scale are the library's.  Nothing is read back."""
    torch = _torch()
    if score not in ROUTE_SCORES:
        raise MtqError(f"score must be one of {tuple(ROUTE_SCORES)}, got {score!r}")
    code, _count, _stride, T, count, ld = _matrix(logits, (2,))
    topk = int(topk)
    if T <= 0 or count <= 0 or topk <= 0:
        raise MtqError("tokens, count and topk must be positive")
    bias_ptr = None
    if bias is not None:
        bias_ptr = _buffer(bias, torch.float32, count, "bias")
        if bias.numel() != count:
            raise MtqError(f"bias must have count = {count} entries, got {bias.numel()}")
    fn = _entry("mtq_moe_route")
    ids, ld_ids = _route_out(out_ids, T, topk, torch.int32, logits.device, "out_ids")
    weights, ld_w = _route_out(out_weights, T, topk, torch.float32, logits.device, "out_weights")
    scores, scores_ptr, ld_scores = None, None, 0
    if return_scores or out_scores is not None:
        scores, ld_scores = _route_out(out_scores, T, count, torch.float32, logits.device, "out_scores")
        scores_ptr = scores.data_ptr()
    check(fn(logits.data_ptr(), code, ld, T, count, topk, ROUTE_SCORES[score], bias_ptr, int(n_group), int(topk_group), int(group_top),
             int(bool(renormalize)), float(eps), float(scale), ids.data_ptr(), ld_ids, weights.data_ptr(), ld_w, scores_ptr, ld_scores,
             _packed_stream_ptr(stream)))
    return ids, weights, scores


def debug_packed_decode(fmt: str):
    """mtq_debug_packed_decode: (got, want) int32 device tensors [16][256][16][16] = [rot][E][q][i] holding the float32 words the skinny
    kernel's decode and the reference decode give code (16 q + (i + rot) % 16) mod 2^bits at element i under exponent byte E."""
    torch = _torch()
    require_gpu()
    if fmt not in ("bfp8", "bfp4", "bfp2"):
        raise MtqError(f"fmt must be bfp8, bfp4 or bfp2, got {fmt!r}")
    got = torch.empty((16, 256, 16, 16), dtype=torch.int32, device="cuda")
    want = torch.empty_like(got)
    check(_entry("mtq_debug_packed_decode")(FMT_CODE[fmt], got.data_ptr(), want.data_ptr(), _stream_ptr()))
    return got, want


def dequant_fp8_block(w, scale_inv):
    """K5: w — 2-D device tensor of float8_e4m3fn (or its uint8 bytes); scale_inv — 2-D float32 block scales →
    float32 device tensor w.float() * scale_inv.repeat_interleave(block) (hf_model_utils.py:209-215)."""
    torch = _torch()
    require_gpu()
    if w.dim() != 2 or scale_inv.dim() != 2 or not w.is_cuda:
        raise MtqError("expected 2-D device tensors")
    wb = w.view(torch.uint8).contiguous()
    sc = scale_inv.to(device=w.device, dtype=torch.float32).contiguous()
    out = torch.empty(wb.shape, dtype=torch.float32, device=w.device)
    check(lib().mtq_dequant_fp8_block(wb.data_ptr(), sc.data_ptr(), wb.shape[0], wb.shape[1], wb.stride(0), sc.shape[0], sc.shape[1],
                                      out.data_ptr(), out.stride(0), _stream_ptr()))
    return out


# ----------------------------------------------------------------------------- host decisions

class GreedyScan:
    """H1: the sequential scan of mixed_tile_greedy.py:133-346 on a host copy of the stats."""

    def __init__(self, stats: np.ndarray, mask: int, metric: str, threshold: float, elem_count: float, base_fmt: str):
        self.stats = np.ascontiguousarray(stats, dtype=np.float64)  # kept alive: the handle reads it
        self.T = self.stats.shape[0]
        self._h = ctypes.c_void_p()
        check(lib().mtq_greedy_create(ctypes.byref(self._h), self.stats.ctypes.data, self.T, mask, METRIC_CODE[metric],
                                      float(threshold), float(elem_count), MIXED_TILE_FORMATS.index(base_fmt)))

    def run_pass(self, fmt: str, order: np.ndarray) -> None:
        order = np.ascontiguousarray(order, dtype=np.int64)
        check(lib().mtq_greedy_pass(self._h, MIXED_TILE_FORMATS.index(fmt), order.ctypes.data, order.size))

    def fixed(self) -> np.ndarray:
        out = np.empty(self.T, dtype=np.uint8)
        check(lib().mtq_greedy_fixed(self._h, out.ctypes.data))
        return out

    def assignment(self) -> np.ndarray:
        out = np.empty(self.T, dtype=np.int8)
        check(lib().mtq_greedy_assignment(self._h, out.ctypes.data))
        return out

    def counts(self) -> dict[str, int]:
        c = (ctypes.c_int64 * 4)()
        check(lib().mtq_greedy_counts(self._h, c))
        return {f: int(c[i]) for i, f in enumerate(MIXED_TILE_FORMATS)}

    def value(self) -> float:
        v = ctypes.c_double()
        check(lib().mtq_greedy_value(self._h, ctypes.byref(v)))
        return v.value

    def close(self) -> None:
        if self._h:
            lib().mtq_greedy_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NumpyCompatRng:
    """mtq_rng: bit-compatible with np.random.default_rng(seed).permutation(n) (tests pin it against NumPy)."""

    def __init__(self, seed: int):
        self._h = ctypes.c_void_p()
        check(lib().mtq_rng_create(ctypes.byref(self._h), int(seed)))

    def permutation(self, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.int64)
        check(lib().mtq_rng_permutation(self._h, int(n), out.ctypes.data))
        return out

    def integers(self, high: int, n: int) -> np.ndarray:
        """≡ rng.integers(0, high, size=n, dtype=np.int64)."""
        out = np.empty(int(n), dtype=np.int64)
        check(lib().mtq_rng_integers(self._h, int(high), int(n), out.ctypes.data))
        return out

    def __del__(self):
        try:
            if self._h:
                lib().mtq_rng_destroy(self._h)
        except Exception:
            pass


def greedy_run(stats: np.ndarray, mask: int, formats, metric: str, threshold: float, elem_count: float, seed: int):
    """H1 end to end in one GIL-free call → (int8[T] map, counts dict, columns dict)."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    T = stats.shape[0]
    fm = _format_codes(formats)
    amap = np.empty(T, dtype=np.int8)
    counts = (ctypes.c_int64 * 4)()
    out = (ctypes.c_double * 9)()
    check(lib().mtq_greedy_run(stats.ctypes.data, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold),
                               float(elem_count), int(seed), amap.ctypes.data, counts, out))
    return amap, {f: int(counts[i]) for i, f in enumerate(MIXED_TILE_FORMATS)}, _columns(out)


SCAN_DEVICE_MAX_TILES = 1 << 22
SCAN_LDS_MAX_TILES = 32768      # csrc/mtq_scan.hip kScanMaxTilesLds: visiting order in LDS up to here, in global scratch above


def device_scan_supported(formats, metric: str, tiles: int) -> bool:
    """What mtq_greedy_scan_device serves (include/mtq.h): the three metrics, distinct formats, tiles up to SCAN_DEVICE_MAX_TILES."""
    return metric in ("pcc", "mae", "atol") and len(set(formats)) == len(formats) and 0 < tiles <= SCAN_DEVICE_MAX_TILES


def device_copy(dst, src) -> None:
    """dst ← src by a kernel on the current stream (mtq_device_copy_2d); dst may be a pinned host tensor, src a device tensor.  Both
    either contiguous with the same number of bytes, or 2-D / 3-D views whose rows (last dimension) are contiguous and whose leading
    dimensions collapse to one pitch."""
    import torch

    if dst.dtype != src.dtype or dst.shape != src.shape:
        raise ValueError("device_copy needs equal shapes and dtypes")
    if dst.numel() == 0:
        return
    esz = dst.element_size()

    def rows_of(t):
        if t.is_contiguous():
            return t.numel() * esz, 1, t.numel() * esz
        if t.dim() < 2 or t.stride(-1) != 1:
            raise ValueError("device_copy needs contiguous rows")
        lead = t.reshape(-1, t.shape[-1]) if all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2)) else None
        if lead is None or lead.data_ptr() != t.data_ptr():
            raise ValueError("device_copy needs one pitch over the leading dimensions")
        return t.shape[-1] * esz, lead.shape[0], lead.stride(0) * esz

    w_d, r_d, p_d = rows_of(dst)
    w_s, r_s, p_s = rows_of(src)
    if r_d == 1 and r_s > 1:      # contiguous on one side: its rows are the other side's rows
        w_d, r_d, p_d = w_s, r_s, w_s
    if r_s == 1 and r_d > 1:
        w_s, r_s, p_s = w_d, r_d, w_d
    check(lib().mtq_device_copy_2d(dst.data_ptr(), p_d, src.data_ptr(), p_s, w_d, r_d, _stream_ptr()))


def greedy_scan_device(stats_dev, mask: int, formats, metric: str, threshold: float, elem_count: float, seeds_dev, maps_out=None,
                       status_out=None, scratch=None, counts_out=None):
    """H1 on the device over FULL records [count, tiles, rec] where K1 wrote them → (int8 [count, tiles] maps, int32 [count]
    status) device tensors, asynchronous on the current stream.  seeds_dev: uint64/int64 device tensor [count]."""
    torch = _torch()
    count, T = int(stats_dev.shape[0]), int(stats_dev.shape[1])
    fm = _format_codes(formats)
    maps = maps_out if maps_out is not None else torch.empty((count, T), dtype=torch.int8, device=stats_dev.device)
    status = status_out if status_out is not None else torch.empty((count,), dtype=torch.int32, device=stats_dev.device)
    need = greedy_scan_scratch_bytes(count, T)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=stats_dev.device)
    elif scratch.numel() < need:   # a caller's slicing bug must not turn into a device allocation per call
        raise ValueError(f"scratch holds {scratch.numel()} bytes, mtq_greedy_scan_scratch_bytes() asks for {need}")
    check(lib().mtq_greedy_scan_device(stats_dev.data_ptr(), count, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold),
                                       float(elem_count), seeds_dev.data_ptr(), maps.data_ptr(), status.data_ptr(),
                                       counts_out.data_ptr() if counts_out is not None else None, scratch.data_ptr(), int(scratch.numel()), _stream_ptr()))
    return maps, status


def scan_orders_device(seed: int, tiles: int, n_orders: int = 2, out=None):
    """The visiting orders every tensor of a launch shares (mtq_scan_orders_device): generator states and the permutations of
    range(tiles) of passes 1 (and 2) for `seed` → uint8 device buffer, asynchronous on the current stream."""
    torch = _torch()
    require_gpu()
    need = int(lib().mtq_scan_orders_bytes(int(tiles)))
    if out is None:
        out = torch.empty((need,), dtype=torch.uint8, device="cuda")
    elif out.numel() < need:
        raise ValueError("orders buffer is smaller than mtq_scan_orders_bytes()")
    check(lib().mtq_scan_orders_device(int(seed), int(tiles), int(n_orders), out.data_ptr(), int(out.numel()), _stream_ptr()))
    return out


EARLY = ("mtq_scan_rank_device", "mtq_tile_stats_partial_begin_early", "mtq_greedy_scan_device_early")


def early_bound() -> bool:
    """Whether this build of the library binds the early form's entries (optional symbols: an older build of the same version lacks them)."""
    return _has(EARLY)


def rank_table_host(perm) -> np.ndarray:
    """What mtq_scan_rank_device computes, restated on the host: rank[perm[i]] = i (uint32) — np.argsort(perm) of a permutation."""
    perm = np.asarray(perm, dtype=np.int64)
    rank = np.full(perm.size, 0xFFFFFFFF, dtype=np.uint32)
    rank[perm] = np.arange(perm.size, dtype=np.uint32)
    return rank


def early_rank_host(seed: int, tiles: int, which: int = 1) -> np.ndarray:
    """The table scan_rank_device(scan_orders_device(seed, tiles), tiles, which) holds, from the library's host generator: the search draws
    one permutation of range(tiles) per pass while every tile is still a candidate; order `which` is the one after `which` + 1 others."""
    rng = NumpyCompatRng(seed)
    for _ in range(int(which) + 1):
        rng.permutation(tiles)
    return rank_table_host(rng.permutation(tiles))


def scan_rank_device(orders, tiles: int, which: int, out=None):
    """mtq_scan_rank_device: the inverse of order `which` (0: pass 1's, 1: pass 2's) of scan_orders_device's buffer → int32 device tensor
    [tiles] holding uint32 ranks, asynchronous on the current stream (which must be ordered behind the orders' launch)."""
    torch = _torch()
    require_gpu()
    if out is None:
        out = torch.empty((int(tiles),), dtype=torch.int32, device=orders.device)
    elif out.numel() < int(tiles) or out.element_size() != 4:
        raise ValueError("rank must hold one 32-bit entry per tile")
    check(_entry("mtq_scan_rank_device")(orders.data_ptr(), int(tiles), int(which), out.data_ptr(), _stream_ptr()))
    return out


def greedy_scan_device_early(stats_dev, mask: int, formats, metric: str, threshold: float, elem_count: float, seeds_dev, maps_out, status_out,
                             scratch, counts_out, orders, listed, n_listed, carry, rank, cutoff: int) -> None:
    """mtq_greedy_scan_device_early: phase 1 of greedy_scan_device_ex behind tile_stats_partial_begin_early with the same rank and cutoff —
    the last pass's candidates ranked below the cutoff stay off the list."""
    count, T = int(stats_dev.shape[0]), int(stats_dev.shape[1])
    if scratch.numel() < greedy_scan_scratch_bytes(count, T):
        raise ValueError("scratch is smaller than mtq_greedy_scan_scratch_bytes()")
    if rank.numel() < T or rank.element_size() != 4:
        raise ValueError("rank must hold one 32-bit entry per tile of a tensor")
    fm = _format_codes(formats)
    check(_entry("mtq_greedy_scan_device_early")(stats_dev.data_ptr(), count, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold), float(elem_count),
                                                 seeds_dev.data_ptr(), maps_out.data_ptr(), status_out.data_ptr(),
                                                 counts_out.data_ptr() if counts_out is not None else None, scratch.data_ptr(), int(scratch.numel()),
                                                 orders.data_ptr() if orders is not None else None, listed.data_ptr(), n_listed.data_ptr(), carry.data_ptr(),
                                                 rank.data_ptr(), int(cutoff), _stream_ptr()))


def greedy_scan_device_ex(stats_dev, mask: int, formats, metric: str, threshold: float, elem_count: float, seeds_dev, maps_out, status_out,
                          scratch, counts_out=None, orders=None, phase: int = 0, listed=None, n_listed=None, carry=None) -> None:
    """mtq_greedy_scan_device_ex: the device search with shared visiting orders (orders: scan_orders_device's buffer for the seed all
    tensors share) and / or in phases (1: every pass but the last + the last pass's candidates → listed / n_listed, state → carry;
    2: the last pass).  Caller-owned buffers throughout; scratch must hold mtq_greedy_scan_scratch_bytes(count, tiles) bytes."""
    count, T = int(stats_dev.shape[0]), int(stats_dev.shape[1])
    need = greedy_scan_scratch_bytes(count, T)
    if scratch.numel() < need:
        raise ValueError("scratch is smaller than mtq_greedy_scan_scratch_bytes()")
    fm = _format_codes(formats)
    check(lib().mtq_greedy_scan_device_ex(stats_dev.data_ptr(), count, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold), float(elem_count),
                                          seeds_dev.data_ptr(), maps_out.data_ptr(), status_out.data_ptr(),
                                          counts_out.data_ptr() if counts_out is not None else None, scratch.data_ptr(), int(scratch.numel()),
                                          orders.data_ptr() if orders is not None else None, int(phase),
                                          listed.data_ptr() if listed is not None else None, n_listed.data_ptr() if n_listed is not None else None,
                                          carry.data_ptr() if carry is not None else None, _stream_ptr()))


def tile_stats_listed(x3d, layout_mask: int, full_mask: int, err_mask: int, listed, n_listed, stats, scratch=None) -> None:
    """mtq_tile_stats_listed: for the tiles listed[0 .. n_listed[0]) (device uint32 / int32 tensors; entries tensor * tiles + tile) the five
    statistics of full_mask's formats and Σ|x−y|, max|x−y| of err_mask's, into stats [count, tiles, rec(layout)] in place.  scratch:
    int32 device tensor of listed.numel() + 1 entries (lets bf16 input take the exact-integer kernel), or None."""
    require_gpu()
    code, count, stride, rows, cols, ld = _contiguous_batch(x3d)
    check(lib().mtq_tile_stats_listed(x3d.data_ptr(), code, count, stride, rows, cols, ld, layout_mask, full_mask, err_mask,
                                      listed.data_ptr(), n_listed.data_ptr(), int(listed.numel()),
                                      scratch.data_ptr() if scratch is not None else None, stats.data_ptr(), _stream_ptr()))


def greedy_run_batch(stats: np.ndarray, mask: int, formats, metric: str, threshold: float, elem_count: float, seeds, n_threads: int):
    """mtq_greedy_run over a [count, tiles, rec] record array on n_threads host threads (one GIL-free call)
    → (int8 [count, tiles] maps, int64 [count, 4] counts, float64 [count, 9] columns+sums)."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    count, T = stats.shape[0], stats.shape[1]
    fm = _format_codes(formats)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    maps = np.empty((count, T), dtype=np.int8)
    counts = np.empty((count, 4), dtype=np.int64)
    outs = np.empty((count, 9), dtype=np.float64)
    check(lib().mtq_greedy_run_batch(stats.ctypes.data, count, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold),
                                     float(elem_count), sd.ctypes.data, maps.ctypes.data, counts.ctypes.data, outs.ctypes.data, int(n_threads)))
    return maps, counts, outs


def _score_rows(mask: int) -> int:
    """Rows of mtq_tile_scores' output: one per format of the mask, the identity bf16 (first) included."""
    return bin(mask & 0xF).count("1") + (1 if (mask & MASK_BF16_IDENTITY) and not (mask & 1) else 0)


def tile_scores(stats: np.ndarray, mask: int, metric: str) -> np.ndarray:
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    T = stats.shape[0]
    out = np.empty((_score_rows(mask), T), dtype=np.float64)
    check(lib().mtq_tile_scores(stats.ctypes.data, T, mask, METRIC_CODE[metric], out.ctypes.data))
    return out


def threshold_assign(stats: np.ndarray, mask: int, formats, metric: str, threshold: float, band: float = 2e-6, with_near: bool = False):
    """K4 on host stats → (int8[T] map, knife-edge tile ids[, uint8 masks of the format codes inside the band per id])."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    T = stats.shape[0]
    fm = _format_codes(formats)
    amap = np.empty(T, dtype=np.int8)
    knife = np.empty(T, dtype=np.int64)
    near = np.empty(T, dtype=np.uint8)
    nk = ctypes.c_int64(0)
    check(lib().mtq_threshold_assign(stats.ctypes.data, T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold), float(band),
                                     amap.ctypes.data, knife.ctypes.data, near.ctypes.data, T, ctypes.byref(nk)))
    k = min(nk.value, T)
    return (amap, knife[:k].copy(), near[:k].copy()) if with_near else (amap, knife[:k].copy())


def tile_scores_device(stats_dev, mask: int, metric: str):
    """mtq_tile_scores on device-resident records [tiles, rec] → device float64 [formats, tiles] (async on the current stream)."""
    torch = _torch()
    require_gpu()
    T = stats_dev.shape[0]
    out = torch.empty((_score_rows(mask), T), dtype=torch.float64, device=stats_dev.device)
    check(lib().mtq_tile_scores_device(stats_dev.data_ptr(), T, mask, METRIC_CODE[metric], out.data_ptr(), _stream_ptr()))
    return out


def threshold_assign_device_raw(stats_dev, mask: int, formats, metric: str, threshold: float, band: float = 2e-6, out=None):
    """K4 on device-resident records [T, rec] (any number of tensors' tiles back to back) → device int8 [2, T]: row 0 the
    map, row 1 the knife-edge masks (bit c: format code c scored inside the band; 0 for most tiles); asynchronous on the
    current stream.  `out`: a pair of contiguous int8 device vectors of T entries each (map, masks) to write instead."""
    torch = _torch()
    require_gpu()
    T = stats_dev.shape[0]
    fm = _format_codes(formats)
    both = torch.empty((2, T), dtype=torch.int8, device=stats_dev.device) if out is None else out
    for row in (both[0], both[1]):
        if row.dtype != torch.int8 or row.numel() != T or not row.is_contiguous() or not row.is_cuda:
            raise ValueError("threshold_assign_device_raw: out must be two contiguous int8 device vectors of one entry per tile")
    check(lib().mtq_threshold_assign_device(stats_dev.data_ptr(), T, mask, fm, len(formats), METRIC_CODE[metric], float(threshold), float(band),
                                            both[0].data_ptr(), both[1].data_ptr(), _stream_ptr()))
    return both


def knife_tiles_device(x3d, near, formats, cap: int, list_out, tiles_out, transposed: bool = False) -> None:
    """The threshold rule's knife-edge tiles, prepared on the device (mtq_knife_tiles_device): `near` = the int8 masks of
    threshold_assign_device_raw for the (count, rows, cols) batch x3d; list_out int64 [cap + 1] ← flat tile ids (any order) and,
    last, how many were flagged; tiles_out float32 [1 + len(formats), cap, 32, 32] ← their values and every format's reconstruction.
    Asynchronous on the current stream.  transposed=True: the same for Xᵀ of every matrix, read in place (mtq_knife_tiles_transposed):
    `near` and the ids follow Xᵀ's grid (K1T's numbering) and the tiles are Xᵀ tiles in Xᵀ's row-major order."""
    code, count, stride, rows, cols, ld = _matrix(x3d, (3,))
    torch = _torch()
    require_gpu()
    th, tw = tiles_hw(cols, rows) if transposed else tiles_hw(rows, cols)
    if near.dtype != torch.int8 or near.numel() != count * th * tw or not near.is_contiguous():
        raise ValueError("near must be a contiguous int8 vector of one entry per tile")
    if list_out.dtype != torch.int64 or list_out.numel() != cap + 1 or not list_out.is_contiguous():
        raise ValueError("list_out must be a contiguous int64 vector of cap + 1 entries")
    if cap and (tiles_out.dtype != torch.float32 or tiles_out.numel() != (1 + len(formats)) * cap * 1024 or not tiles_out.is_contiguous()):
        raise ValueError("tiles_out must be a contiguous float32 tensor of (1 + formats) x cap x 32 x 32")
    fm = _format_codes(formats) if formats else None
    fn = _entry("mtq_knife_tiles_transposed") if transposed else lib().mtq_knife_tiles_device
    check(fn(x3d.data_ptr(), code, count, stride, rows, cols, ld, near.data_ptr(), fm, len(formats), int(cap), list_out.data_ptr(),
             tiles_out.data_ptr() if cap else None, _stream_ptr()))


def threshold_assign_device(stats_dev, mask: int, formats, metric: str, threshold: float, band: float = 2e-6, with_near: bool = False):
    """K4 on device-resident records → (int8[T] map on the host, knife-edge tile ids[, their near masks]): only T + T bytes
    cross PCIe."""
    host = threshold_assign_device_raw(stats_dev, mask, formats, metric, threshold, band).cpu().numpy()
    ids = np.flatnonzero(host[1]).astype(np.int64)
    return (host[0].copy(), ids, host[1][ids].astype(np.uint8)) if with_near else (host[0].copy(), ids)


def columns_from_sums(sums7: np.ndarray, elem_count: float) -> dict:
    """pcc / mae / atol from Σx, Σx², Σy, Σy², Σxy, Σ|d|, max|d| (mtq_columns_from_sums)."""
    sums = np.ascontiguousarray(sums7, dtype=np.float64)
    out = (ctypes.c_double * 9)()
    check(lib().mtq_columns_from_sums(sums.ctypes.data, float(elem_count), out))
    return _columns(out)


def columns_from_stats_device(stats_dev, mask: int, assignment, elem_count: float) -> dict:
    """Tensor-level pcc / mae / atol of the reconstruction `assignment` implies, summed on the device from device-resident
    records (fixed tree order); the map goes up (1 B/tile), seven doubles come back."""
    torch = _torch()
    require_gpu()
    T = stats_dev.shape[0]
    if isinstance(assignment, np.ndarray):
        amap = torch.from_numpy(np.ascontiguousarray(assignment, dtype=np.int8).reshape(-1)).to(stats_dev.device)
    else:
        amap = assignment.reshape(-1).to(device=stats_dev.device, dtype=torch.int8).contiguous()
    if amap.numel() != T:
        raise MtqError("assignment has the wrong number of tiles")
    scratch = torch.empty(columns_scratch_doubles(), dtype=torch.float64, device=stats_dev.device)
    check(lib().mtq_column_sums_device(stats_dev.data_ptr(), T, mask, amap.data_ptr(), scratch.data_ptr(), _stream_ptr()))
    sums = np.ascontiguousarray(scratch[:7].cpu().numpy())
    if np.isnan(sums[0]) and not np.isnan(sums[1]):
        raise MtqError("map names a format that is not in fmt_mask")
    return columns_from_sums(sums, elem_count)


def columns_from_stats(stats: np.ndarray, mask: int, assignment: np.ndarray, elem_count: float) -> dict:
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    a = np.ascontiguousarray(assignment, dtype=np.int8).reshape(-1)
    out = (ctypes.c_double * 9)()
    check(lib().mtq_columns_from_stats(stats.ctypes.data, stats.shape[0], mask, a.ctypes.data, float(elem_count), out))
    return _columns(out)


# ----------------------------------------------------------------------------- the streamed drivers' launches
# Called once per chunk or batch: the streams are explicit (each call site picks its own), and the checks read attributes only — no
# device query, allocation, copy or synchronisation.  Buffers are views of grow-only storage, so their sizes are lower bounds.

@functools.lru_cache(maxsize=None)
def columns_scratch_doubles() -> int:
    """Doubles of column-sum scratch per tensor (mtq_columns_scratch_doubles: a constant of the library)."""
    return int(lib().mtq_columns_scratch_doubles())


def greedy_scan_scratch_bytes(count: int, tiles: int) -> int:
    return int(lib().mtq_greedy_scan_scratch_bytes(int(count), int(tiles)))


def scan_carry_bytes(count: int) -> int:
    return int(lib().mtq_scan_carry_bytes(int(count)))


def _sums_ptrs(stats, count: int, T: int, mask: int, maps, scratch, sums_host=None) -> tuple:
    """The pointers of a column-sum launch over `count` tensors of T tiles in all, checked: full records (2 + 5 doubles per format of
    mask), a map entry per tile, columns_scratch_doubles() of scratch per tensor and, for the threshold calls, 11 doubles per tensor."""
    torch = _torch()
    return (_buffer(stats, torch.float64, T * record_doubles(mask & ~MASK_SLIM), "records"), _buffer(maps, torch.int8, T, "maps"),
            _buffer(scratch, torch.float64, count * columns_scratch_doubles(), "scratch"),
            None if sums_host is None else _buffer(sums_host, torch.float64, count * 11, "sums_host", device=False))


def column_sums_device_batched(stats, count: int, tiles: int, mask: int, maps, scratch, stream) -> None:
    """mtq_column_sums_device_batched on `stream`: the seven column sums of `count` tensors' maps [count, tiles] over their records
    → scratch [count, columns_scratch_doubles()], tensor i's sums at the head of row i."""
    sp, mp, wp, _ = _sums_ptrs(stats, count, count * tiles, mask, maps, scratch)
    check(lib().mtq_column_sums_device_batched(sp, count, tiles, mask, mp, wp, _stream(stream)))


def threshold_columns(stats, count: int, tiles: int, dec_mask: int, maps, scratch, sums_host, stream) -> None:
    """mtq_threshold_columns on `stream`: column_sums_device_batched, then every tensor's seven sums and its tile count per format
    into the pinned sums_host [count, 11]."""
    sp, mp, wp, hp = _sums_ptrs(stats, count, count * tiles, dec_mask, maps, scratch, sums_host)
    check(lib().mtq_threshold_columns(sp, count, tiles, dec_mask, mp, wp, hp, _stream(stream)))


def threshold_columns_ragged(stats, tiles_per, dec_mask: int, maps, scratch, sums_host, stream) -> None:
    """mtq_threshold_columns_ragged: threshold_columns for a ragged group, matrix j's tiles_per[j] tiles behind matrix j-1's."""
    n = len(tiles_per)
    sp, mp, wp, hp = _sums_ptrs(stats, n, sum(tiles_per), dec_mask, maps, scratch, sums_host)
    check(lib().mtq_threshold_columns_ragged(sp, (ctypes.c_int64 * n)(*tiles_per), n, dec_mask, mp, wp, hp, _stream(stream)))


def _enqueue_ptrs(count: int, T: int, k1_mask: int, formats, stats, both_dev, both_host, cap: int, list_dev, knife_dev, list_host,
                  scratch, sums_host) -> tuple:
    """The arguments of mtq_threshold_enqueue(_ragged) from records to sums_host for `count` tensors of T tiles in all, checked."""
    torch = _torch()
    return (_buffer(stats, torch.float64, T * record_doubles(k1_mask & ~MASK_SLIM), "records"), _buffer(both_dev, torch.int8, 2 * T, "both_dev"),
            _buffer(both_host, torch.int8, 2 * T, "both_host", device=False), int(cap), _buffer(list_dev, torch.int64, cap + 1, "list_dev"),
            _buffer(knife_dev, torch.float32, (1 + len(formats)) * cap * 1024, "knife_dev") if cap else None,
            _buffer(list_host, torch.int64, cap + 1, "list_host", device=False),
            None if scratch is None else _buffer(scratch, torch.float64, count * columns_scratch_doubles(), "scratch"),
            None if sums_host is None else _buffer(sums_host, torch.float64, count * 11, "sums_host", device=False))


def threshold_enqueue(x3d, k1_mask: int, dec_mask: int, formats, metric: str, threshold: float, band: float, stats, both_dev, both_host,
                      cap: int, list_dev, knife_dev, list_host, scratch, sums_host, stream, side_stream, transposed: bool = False) -> None:
    """One batch (count, rows, cols) of the streamed threshold driver as one call (mtq_threshold_enqueue; transposed: the search of Xᵀ,
    mtq_threshold_enqueue_transposed): K1 → records, K4 → both_dev [2, T] (maps, knife-edge masks) and its pinned mirror both_host on
    `stream`; the knife-edge list (list_dev, list_host [cap + 1]) and tiles (knife_dev [1 + formats, cap, 32, 32]) on side_stream (None:
    on `stream`); with scratch and sums_host, the column sums under K4's maps on `stream` (threshold_columns)."""
    code, count, stride, rows, cols, ld = _matrix(x3d, (3,))
    th, tw = tiles_hw(rows, cols)
    ptrs = _enqueue_ptrs(count, count * th * tw, k1_mask, formats, stats, both_dev, both_host, cap, list_dev, knife_dev, list_host,
                         scratch, sums_host)
    fn = _entry("mtq_threshold_enqueue_transposed") if transposed else lib().mtq_threshold_enqueue
    check(fn(x3d.data_ptr(), code, count, stride, rows, cols, ld, k1_mask, dec_mask, _format_codes(formats), len(formats), METRIC_CODE[metric],
             threshold, band, *ptrs, _stream(stream), _stream(side_stream)))


def threshold_enqueue_ragged(mats, k1_mask: int, dec_mask: int, formats, metric: str, threshold: float, band: float, stats, both_dev,
                             both_host, cap: int, list_dev, knife_dev, list_host, scratch, sums_host, stream, side_stream) -> list[int]:
    """threshold_enqueue for a ragged group (mtq_threshold_enqueue_ragged): 2-D matrices of one storage type and any shapes, their
    tiles numbered through → the tiles of every matrix."""
    arr, code, tiles_per = ragged_matrices(mats)
    ptrs = _enqueue_ptrs(len(mats), sum(tiles_per), k1_mask, formats, stats, both_dev, both_host, cap, list_dev, knife_dev, list_host,
                         scratch, sums_host)
    check(lib().mtq_threshold_enqueue_ragged(arr, len(mats), code, k1_mask, dec_mask, _format_codes(formats), len(formats), METRIC_CODE[metric],
                                             threshold, band, *ptrs, _stream(stream), _stream(side_stream)))
    return tiles_per
