"""The MoE routing cases that tests/test_packed_moe_gpu.py (the kernels of csrc/mtq_moe.hip) and tests/test_packed_moe_host.py (the
emulation) both draw: the routings, the want-side of plan, dispatch and combine in NumPy, and the copy kernels' launch geometry
written out once more, so that a test can state in code which path and which trip of a loop its shape meets.  NumPy only: no
fixture, no device.

  routing kinds  "uniform"; "one": every slot on the last expert; "twice": slot 1 of every token repeats slot 0; "dropped": about a
                 quarter of the ids replaced by -1, count, count + 7, -count and the id type's extremes; "none_live": every id one of
                 those (R = 0); "distinct": slot s names expert s % count, so with count >= 64 a 64-slot step holds 64 different
                 experts; "high_word" (int64 only): about a quarter of the ids are a live id +- 2^32, slot 0 is 2^32 itself - all
                 dropped, and all live to a read that keeps the low 32 bits.
"""
from __future__ import annotations

import functools

import numpy as np

SENTINEL = 0xA5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
KINDS = ("uniform", "one", "twice", "dropped", "none_live", "distinct", "high_word")
ROUTINGS = ((1, 1, 1), (1, 8, 256), (7, 2, 5), (64, 8, 256), (128, 8, 256), (129, 8, 256), (300, 6, 300), (4099, 8, 256),
            (16, 64, 4096), (17, 64, 4096), (1025, 1, 1), (256, 8, 256), (1024, 8, 64), (1025, 8, 64))
RUN = 1024                                                # include/mtq.h MTQ_MOE_RUN: the slots of one run
COPY_THREADS, MAX_BLOCKS = 256, 8192                      # csrc/mtq_moe.hip kCopyThreads, kMaxBlocks


def _bf16_words(a32: np.ndarray) -> np.ndarray:
    """float32 (finite) → the bf16 words of its round-to-nearest-even, as int16."""
    u = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def _bf16_valued(a32: np.ndarray) -> np.ndarray:
    return (_bf16_words(a32).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


# ----------------------------------------------------------------------------- the launch geometry, as the host code of mtq_moe.hip has it

def lanes_log2_of(chunks: int, least_log2: int) -> int:
    lg = least_log2
    while lg < 8 and (1 << lg) < chunks:
        lg += 1
    return lg


def dispatch_geometry(k: int, vec: bool):
    """(L, rows per workgroup, trips of lane 0 through a row's chunks): 8 elements a chunk on the 16-byte path, one on the element path."""
    chunks = k // 8 if vec else k
    lg = lanes_log2_of(chunks, 0)
    return 1 << lg, COPY_THREADS >> lg, -(-chunks // (1 << lg))


def combine_geometry(n: int):
    """(L, tokens per workgroup, trips of lane 0 through the columns): a lane owns 8 columns a trip on either path."""
    chunks = (n + 7) // 8
    lg = lanes_log2_of(chunks, 6)
    return 1 << lg, COPY_THREADS >> lg, -(-chunks // (1 << lg))


def plan_scan_per(count: int, one_launch: bool) -> int:
    """scan_counts' experts per thread: one wave in the one-launch kernel, 256 threads in the scan kernel."""
    threads = 64 if one_launch else 256
    return -(-count // threads)


# ----------------------------------------------------------------------------- plan

def _routing(T, K, count, kind, np_type, seed=0) -> np.ndarray:
    rng = np.random.default_rng(1000 * T + 10 * K + count + seed)
    ids = rng.integers(0, count, size=(T, K)).astype(np_type)
    info = np.iinfo(np_type)
    if kind == "one":
        ids[:] = count - 1
    elif kind == "twice" and K > 1:
        ids[:, 1] = ids[:, 0]
    elif kind == "dropped":
        bad = np.array([-1, count, info.min, info.max, count + 7, -count], dtype=np_type)
        drop = rng.random((T, K)) < 0.25
        drop.reshape(-1)[0] = True
        ids[drop] = bad[rng.integers(0, bad.size, size=int(drop.sum()))]
    elif kind == "none_live":
        bad = np.array([-1, count, info.min, info.max, count + 7], dtype=np_type)
        ids[:] = bad[rng.integers(0, bad.size, size=(T, K))]
    elif kind == "distinct":
        ids.reshape(-1)[:] = np.arange(T * K) % count
    elif kind == "high_word":
        assert np_type == np.int64, "an int32 id has no high word"
        far = rng.random((T, K)) < 0.25
        ids[far] += np.where(rng.random(int(far.sum())) < 0.5, 2 ** 32, -2 ** 32)
        ids.reshape(-1)[0] = 2 ** 32
    else:
        assert kind in ("uniform", "twice"), kind
    return ids


def _want_plan(ids: np.ndarray, count: int):
    """(group_rows, row_of, src) by the contract's independent statement: the stable argsort of where(live, id, count)."""
    flat = ids.astype(np.int64).reshape(-1)
    S = flat.size
    live = (flat >= 0) & (flat < count)
    order = np.argsort(np.where(live, flat, count), kind="stable")
    R = int(live.sum())
    src = np.full(S, -1, dtype=np.int32)
    src[:R] = order[:R]
    row_of = np.full(S, -1, dtype=np.int32)
    row_of[order[:R]] = np.arange(R, dtype=np.int32)
    group_rows = np.zeros(count + 1, dtype=np.int32)
    group_rows[1:] = np.cumsum(np.bincount(flat[live], minlength=count))
    return group_rows, row_of, src


def check_kind(kind: str, ids: np.ndarray, count: int, want) -> None:
    """What a routing kind promises, asserted on the want-side, so that a case which lost its point fails before the device is asked."""
    group_rows, row_of, src = want
    flat = ids.astype(np.int64).reshape(-1)
    S = flat.size
    if kind == "one":
        assert group_rows[-1] == S and np.array_equal(src, np.arange(S))
    elif kind == "dropped":
        assert group_rows[-1] < S
    elif kind == "none_live":
        assert not group_rows.any() and (row_of == -1).all() and (src == -1).all()                 # R = 0
    elif kind == "distinct" and count >= 64:
        steps = flat[: S // 64 * 64].reshape(-1, 64)                                                # the ragged last step holds fewer
        assert all(np.unique(step).size == 64 for step in steps)
        if S <= count:
            assert np.array_equal(row_of, np.arange(S))
    elif kind == "high_word":
        out = (flat < 0) | (flat >= count)
        looks_live = out & ((flat & 0xFFFFFFFF) < count)   # the low word alone is an expert
        assert flat[0] == 2 ** 32 and looks_live[0] and (S < 16 or looks_live.sum() > 1)
        assert (row_of[out] == -1).all() and group_rows[-1] == S - out.sum() < S


# ----------------------------------------------------------------------------- dispatch

DT, DK = 37, 3                                            # 111 rows: more than one workgroup at every k of the path tests
NEVER = np.uint16(0x7FC1)                                 # the word behind x in the tests: x holds it nowhere, so no output may


@functools.lru_cache(maxsize=None)
def _dispatch_case(k, T=DT, K=DK, far=None):
    """(x words, src, want words).  src: random over [0, S) with -1, S, S + 5 and the int32 extremes by hand; `far`: a row from which
    two of the five stand (the last row is one of them), for the grids that stride."""
    S = T * K
    rng = np.random.default_rng(k)
    x = rng.integers(0, 1 << 16, size=(T, k), dtype=np.uint16).astype(np.uint16)          # any words: a bit copy, NaN words included
    x[x == NEVER] = 1
    src = rng.integers(0, S, size=S).astype(np.int64)
    at = [0, 5, 17, 40 if far is None else far + 3, S - 1]
    assert far is None or far <= at[3] < at[4]
    src[at] = [-1, S, I32_MIN, I32_MAX, S + 5]
    src[1], src[2] = S - 1, 0
    keep = (src >= 0) & (src < S)
    assert keep.sum() == S - 5
    want = np.zeros((S, k), dtype=np.uint16)
    want[keep] = x[src[keep] // K]
    return x, src.astype(np.int32), want


# ----------------------------------------------------------------------------- combine

CT, CK = 19, 4
POISON = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0xFFC00000], dtype=np.uint32).view(np.float32)


def _weights(rng, T, K):
    w = rng.standard_normal((T, K)).astype(np.float32)
    w[rng.random((T, K)) < 0.2] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _combine_case(n, K=CK, T=CT):
    """Routing with drops, hand-made bad rows, weights, ys (float32 values that are bf16 values, so both storages hold them), bases.
    From K = 5 on, token T - 2 has slots 0 .. 3 dropped and the rest live, token T - 1 the other way round, all with weights that are
    not zero: the sums of those two tokens come from one batch of four slots alone."""
    S = T * K
    rng = np.random.default_rng(n)
    ids = _routing(T, K, 6, "dropped", np.int64, seed=n)
    if K >= 5:
        ids[T - 2, :4], ids[T - 2, 4:] = [-1, 6, 13, -6], np.arange(K - 4) % 6
        ids[T - 1, :4], ids[T - 1, 4:] = [5, 0, 0, 3], -1
    _g, row_of, _s = _want_plan(ids, 6)
    R = int((row_of >= 0).sum())
    assert 0 < R < S
    row_of = row_of.copy()
    live = np.flatnonzero(row_of >= 0)
    assert live.size > 9 and live[9] < (T - 2) * K
    row_of[live[[1, 4, 9]]] = [S, I32_MIN, I32_MAX]        # hand-made: skipped like the dropped slots
    w = _weights(rng, T, K)
    w[0, 0], w[1, 1 % K] = -1.5, 0.0
    if K >= 5:
        w[T - 2:] = np.where(w[T - 2:] == 0, np.float32(0.75), w[T - 2:])
        first, second = row_of.reshape(T, K)[T - 2:, :4], row_of.reshape(T, K)[T - 2:, 4:]
        assert (first[0] < 0).all() and (second[0] >= 0).all() and (first[1] >= 0).all() and (second[1] < 0).all()
    assert (w < 0).any() and (w == 0).any()
    ys = _bf16_valued(rng.standard_normal((S, n)).astype(np.float32) * 3)
    base = _bf16_valued(rng.standard_normal((T, n)).astype(np.float32))
    ys_dev = ys.copy()
    ys_dev[R:] = POISON[rng.integers(0, 4, size=(S - R, n))]                  # never read: no kept slot names a row from R on
    return row_of, w, ys, ys_dev, base


@functools.lru_cache(maxsize=None)
def _combine_permuted_case(n, T, K, far):
    """For the grids that stride: row_of a random permutation of the slots (every row of ys is some slot's) with the hand-made bad
    entries, three of them on tokens from `far` on.  (row_of, w, ys, base); the rows that lost their slot hold poison."""
    S = T * K
    rng = np.random.default_rng(n + T)
    row_of = rng.permutation(S).astype(np.int64)
    at = np.array([0, 7, far * K, (far + 1) * K + K - 1, S - 1])
    assert far < T - 2
    lost = row_of[at].copy()
    row_of[at] = [-1, S, I32_MIN, I32_MAX, S + 5]
    w = _weights(rng, T, K)
    w[far + 2:] = np.where(w[far + 2:] == 0, np.float32(-0.5), w[far + 2:])
    ys = _bf16_valued(rng.standard_normal((S, n)).astype(np.float32) * 3)
    ys[lost] = POISON[rng.integers(0, 4, size=(lost.size, n))]
    base = _bf16_valued(rng.standard_normal((T, n)).astype(np.float32))
    return row_of.astype(np.int32), w, ys, base


def _want_combine(row_of, w, ys, base, T, K):
    """The contract's loop in NumPy's float32: product and sum rounded separately, j ascending, rows outside [0, S) skipped."""
    S = T * K
    acc = np.zeros((T, ys.shape[1]), dtype=np.float32) if base is None else base.astype(np.float32).copy()
    for t in range(T):
        for j in range(K):
            r = int(row_of[t * K + j])
            if 0 <= r < S:
                acc[t] = acc[t] + np.float32(w[t, j]) * ys[r]
    assert acc.dtype == np.float32 and np.isfinite(acc).all()
    return acc
