"""What tests/test_packed_glu_chunked_host.py and tests/test_packed_glu_chunked_gpu.py share: the names of include/mtq_glu_chunked.h with
their walking parents, the routings of the GPU file, and the host arithmetic of the chunked frame written out once more, so that a test
can state in code which path a shape meets.  NumPy only: no fixture, no device.

  plan_bytes      the plan region at the head of every chunked workspace: (count + 1) int32, rounded up to 16.
  clamp / chunks  the kernels' clamp of group_rows into [0, T] and the chunk counts and prefix the plan kernel writes from it.
  slots           the host's bound on the chunk count, from (T, count) alone: floor((T + 31 min(count, T)) / 32).
"""
from __future__ import annotations

import numpy as np

CHUNK = 32                                                # rows of X a wave takes
REDUCE_COLUMNS = 256                                      # columns a workgroup of the reduces owns
HANDOUT = 64                                              # tiles a skinny run loads the tables of at once

GLU = ("mtq_packed_glu_skinny_grouped_chunked", "mtq_packed_glu_matmul_skinny_grouped_chunked")
GATHER = ("mtq_packed_glu_skinny_grouped_chunked_gather", "mtq_packed_glu_matmul_skinny_grouped_chunked_gather")
COMBINE = ("mtq_packed_linear_skinny_grouped_chunked_combine", "mtq_packed_matmul_skinny_grouped_chunked_combine")
ENTRIES = GLU + GATHER + COMBINE
SIZES = tuple(name + "_workspace_bytes" for name in ENTRIES)
NEW = ENTRIES + SIZES                                     # the twelve names
PARENT = {name: name.replace("_chunked", "") for name in NEW}     # the walking entry each one follows

# group_rows of the GPU file's routings (count = len - 1)
ORDINARY = (0, 3, 3, 35, 36, 70)
HOT = (0, 0, 130, 131, 200, 200)                          # a group of 4 * 32 + 2 rows; 9 chunks in 11 slots
EXACT = (0, 33, 66, 99)                                   # count 3: every group one row into a second chunk, the slot bound met exactly
SINGLE = (0, 0, 0, 1, 1, 1)
ROUTINGS = (ORDINARY, HOT, EXACT, SINGLE)


def plan_bytes(count: int) -> int:
    return ((count + 1) * 4 + 15) // 16 * 16


def clamp(group_rows, T: int):
    """(r0, r1) per group as the kernels clamp them: r0 into [0, T], r1 into [r0, T]."""
    g = np.asarray(group_rows, dtype=np.int64)
    r0 = np.clip(g[:-1], 0, T)
    return r0, np.clip(g[1:], r0, T)


def chunks(group_rows, T: int) -> np.ndarray:
    """cstart[0 .. count]: the exclusive prefix of the groups' chunk counts."""
    r0, r1 = clamp(group_rows, T)
    return np.concatenate([[0], np.cumsum((r1 - r0 + CHUNK - 1) // CHUNK)])


def slots(T: int, count: int) -> int:
    return (T + (CHUNK - 1) * min(count, T)) // CHUNK


def chunk_rows(group_rows, T: int):
    """[(group, first row, rows)] of every chunk in slot order."""
    r0, r1 = clamp(group_rows, T)
    return [(e, int(a), int(min(CHUNK, r1[e] - a))) for e in range(len(r0)) for a in range(int(r0[e]), int(r1[e]), CHUNK)]
