"""What tests/test_packed_moe_fused_host.py and tests/test_packed_moe_fused_gpu.py share: the experts of the layer cases in both
orientations, and the host arithmetic of the grouped skinny entries written out once more, so that a test can state in code which
path a shape meets.  NumPy and the emulation only: no fixture, no device.

  rows / transpose   The SAME weights in both orientations: stored="rows" packs W (n, k) with pack_batch, stored="transpose" packs Wᵀ
                     (k, n) with pack_batch_transposed under the transposed map, so a layer of either kind multiplies by one matrix.
  effective_split    a size function's answer divided by the bytes of one float32 (S, n) slice (the issue's rule), 1 where the
                     staged entry's function answers 0 (it needs no workspace at an effective split of 1).
"""
from __future__ import annotations

import functools

import numpy as np

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen
from tests.packed_cases import random_map

COUNT, K_IN, HIDDEN, K_OUT = 5, 128, 96, 64               # the layer of DESIGN.md §A.6w
STORED = ("rows", "transpose")
CHUNK = 32                                                # rows of X a grouped skinny wave takes at a time
REDUCE_COLUMNS = 256                                      # columns a workgroup of the grouped reduces owns


def _weights(count, n, k, seed):
    return np.stack([gen("heavy_f32", seed + i, (n, k)) for i in range(count)])


def pack_experts(w, seed, stored, backend="emulation"):
    """`count` (n, k) weights → the list of packed experts of one orientation; a different random map per expert."""
    count, n, k = w.shape
    if stored == "rows":
        maps = np.stack([random_map((n, k), seed + i) for i in range(count)])
        return packed.pack_batch(_on(w, backend), maps, backend=backend)
    maps = np.stack([random_map((k, n), seed + i) for i in range(count)])
    return packed.pack_batch_transposed(_on(w, backend), maps, backend=backend)      # takes W (count, n, k) and packs the transposes


def _on(a, backend):
    if backend == "emulation":
        return a
    import torch

    return torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def layer_experts(stored, backend="emulation", count=COUNT, k_in=K_IN, hidden=HIDDEN, k_out=K_OUT):
    """(gate, up, down) lists of the layer's experts."""
    return (pack_experts(_weights(count, hidden, k_in, 30), 33, stored, backend), pack_experts(_weights(count, hidden, k_in, 40), 43, stored, backend),
            pack_experts(_weights(count, k_out, hidden, 50), 53, stored, backend))


def effective_split(size_bytes: int, S: int, n: int) -> int:
    """The slices of a float32 [split][S][n] workspace of `size_bytes` (a multiple of 16 at or above them)."""
    one = S * n * 4
    assert size_bytes % 16 == 0 and size_bytes >= 0
    return max(1, size_bytes // one)


def down_split(S: int, count: int, n: int, k: int, split: int) -> int:
    """The effective split of the grouped skinny down projection, from the STAGED entry's size function: 0 bytes is a split of 1."""
    return effective_split(hb.packed_linear_skinny_grouped_workspace_bytes(S, count, n, k, split), S, n)


def glu_split(S: int, count: int, n: int, k: int, split: int) -> int:
    """The effective split of the grouped skinny GLU: its workspace holds both projections at every split."""
    size = hb.packed_glu_skinny_grouped_workspace_bytes(S, count, n, k, split)
    return effective_split(size, S, 2 * n)


def x_vec(ptr: int, ldx: int) -> bool:
    """The skinny kernels' 16-byte X loads: x 16-byte aligned and every row a multiple of 8 elements apart (csrc x_vec_of)."""
    return ptr % 16 == 0 and ldx % 8 == 0
