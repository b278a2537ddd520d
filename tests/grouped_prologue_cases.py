"""Shared by test_packed_grouped_prologue_host.py and _gpu.py: exact-arithmetic inputs for the grouped prologue and the plain float64
reference - the Hadamard matrix product, the exact per-expert shift, float64 matmul with unpack's Ŵ, then the activation and the combine
in moe_combine's order.  x in {-1, 0, 1} with 8 non-zeros per block and an even log2(block) make X′ a multiple of 2^-5 up to 8 in
size, X″ a multiple of 2^-12; Ŵ is small integers (halves under the narrow formats), so every sum below is exact in float32 in any
order (exact_bits asserts it) and the float64 value rounded once is the only right answer."""
import functools

import numpy as np
import torch

from quantization_analysis_amd import packed

COUNT, N, K = 3, 96, 2048                     # three tile rows: the workgroup's fourth wave has none
GROUP_ROWS = np.array([0, 0, 1, 34])          # an empty expert, a one-row chunk, a full chunk and a one-row chunk
CASES = [(0, True), (64, False), (64, True), (256, False), (256, True), (1024, False), (1024, True)]   # (block, shifts)


def exact_x(rng, rows, block):
    x = np.zeros((rows, K), dtype=np.float32)
    B = block or 64
    for r in range(rows):
        for b in range(K // B):
            x[r, b * B + rng.choice(B, 8, replace=False)] = rng.choice((-1.0, 1.0), 8)
    return torch.from_numpy(x).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def experts(seed, mixed, backend):
    """COUNT packed (N, K) experts of integers in [-1, 1] under an all-bf16 or a mixed map → (list of PackedTensor, float64 Ŵ)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-1, 2, (COUNT, N, K)).astype(np.float32)
    maps = (rng.integers(0, 4, (COUNT, N // 32, K // 32)) if mixed else np.zeros((COUNT, N // 32, K // 32))).astype(np.int8)
    host = packed.pack_batch(w, maps, backend="emulation")
    what = np.stack([np.asarray(packed.unpack(pt, backend="emulation"), dtype=np.float64) for pt in host])
    assert np.array_equal(2 * what, np.rint(2 * what)) and np.abs(what).max() <= 1
    return (host if backend == "emulation" else packed.pack_batch(torch.from_numpy(w).cuda(), maps, backend="hip")), what


def exact_bits(a, w):
    """log2 of the largest sum_k |a||w| of an output in units of 2^-13 (half the unit of X″ times Ŵ's halves): below 24, every partial
    sum of a @ w.T is exact in float32 in any order."""
    return float(np.log2((np.abs(a) @ np.abs(w).T).max() * 2.0 ** 13))


def x2_ref(x, owner, block, p):
    """X″ in float64: x·H_block·2^(-log2(block)/2), then the exact shift by the owner's row of p."""
    x = x.double().numpy()
    if block:
        H = np.ones((1, 1))
        while H.shape[0] < block:
            H = np.block([[H, H], [H, -H]])
        x = (x.reshape(x.shape[0], -1, block) @ H).reshape(x.shape[0], -1) * 2.0 ** (-np.log2(block) / 2)
    return x if p is None else np.ldexp(x, -p[owner])


def grouped_ref(x, group_rows, block, p, *whats):
    """Per expert X″·Ŵᵀ over its rows for each Ŵ in whats → float64 (T, N) each; rows of no group stay zero."""
    g = np.asarray(group_rows)
    owner = np.clip(np.searchsorted(g[1:], np.arange(x.shape[0]), side="right"), 0, COUNT - 1)
    x2 = x2_ref(x, owner, block, p)
    ys = [np.zeros((x.shape[0], N)) for _ in whats]
    for e in range(COUNT):
        for y, what in zip(ys, whats):
            y[g[e]: g[e + 1]] = x2[g[e]: g[e + 1]] @ what[e].T
            assert g[e] == g[e + 1] or exact_bits(x2[g[e]: g[e + 1]], what[e]) < 24
    return ys


def combine_ref(ys, row_of, weights, base):
    """moe_combine's stated order in float64: from base, slot by slot, a dropped slot skipped."""
    T, topk = weights.shape
    acc = np.zeros((T, N)) if base is None else base.astype(np.float64).copy()
    for j in range(topk):
        for t in range(T):
            r = row_of[t * topk + j]
            if 0 <= r < T * topk:
                acc[t] += float(weights[t, j]) * ys[r]
        assert np.abs(acc).max() * 2.0 ** 14 < 2 ** 24       # weights in {0.5, 1}: every running sum is exact in float32
    return acc


ENTRIES = ("glu_grouped_skinny", "linear_grouped", "moe_glu", "moe_down_combine", "moe_down_combine_base")
GLU_IDS = [[0, 2], [1, 1], [2, 7], [0, 1], [2, 2]]                  # an id outside [0, COUNT), two tokens naming an expert twice
DOWN_IDS = [[1, 5]] + [[2, 2]] * 16 + [[2, 5]]                     # 36 slots, two dropped: 0, 1 and 33 rows


def run(entry, block, shifts, mixed, backend, prologue, split=0):
    """One entry on the exact inputs → (its float32 result, the float64 reference rounded once to float32), as float64 arrays."""
    rng = np.random.default_rng(block + shifts)
    p = rng.integers(0, 8, (COUNT, K)) if shifts else None
    dev = (lambda t: t.cuda()) if backend == "hip" else (lambda t: t)
    host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    kw = dict(rotate=block, in_exponents=p, prologue=prologue, split=split, backend=backend, out_dtype="float32")
    (gate, wg), (up, wu), (down, wd) = (experts(s, mixed, backend) for s in (1, 2, 3))
    if entry == "glu_grouped_skinny":
        x = exact_x(rng, 34, block)
        got = packed.glu_grouped_skinny(dev(x), GROUP_ROWS, gate, up, act="none", **kw)
        g, u = grouped_ref(x, GROUP_ROWS, block, p, wg, wu)
        want = g * u
    elif entry == "linear_grouped":
        x = exact_x(rng, 34, block)
        got = packed.linear_grouped(dev(x), GROUP_ROWS, down, **kw)
        want, = grouped_ref(x, GROUP_ROWS, block, p, wd)
    elif entry == "moe_glu":
        x = exact_x(rng, len(GLU_IDS), block)
        plan = packed.moe_plan(dev(torch.tensor(GLU_IDS)), COUNT, backend=backend)
        got = packed.moe_glu(dev(x), plan, gate, up, act="none", **kw)
        src = host(plan.src).astype(np.int64)
        xs = torch.where(torch.from_numpy(src >= 0)[:, None], x[np.maximum(src, 0) // 2], torch.zeros((), dtype=x.dtype))
        g, u = grouped_ref(xs, host(plan.group_rows), block, p, wg, wu)
        want = g * u
    else:
        T = len(DOWN_IDS)
        h = exact_x(rng, 2 * T, block)
        plan = packed.moe_plan(dev(torch.tensor(DOWN_IDS)), COUNT, backend=backend)
        assert np.array_equal(host(plan.group_rows), GROUP_ROWS)
        weights = torch.from_numpy(rng.choice((0.5, 1.0), (T, 2)).astype(np.float32))
        base = torch.from_numpy(rng.integers(-4, 5, (T, N)).astype(np.float32)) if entry.endswith("base") else None
        got = packed.moe_down_combine(dev(h), dev(weights), plan, down, base=None if base is None else dev(base), expert_dtype="float32", **kw)
        ys, = grouped_ref(h, GROUP_ROWS, block, p, wd)
        want = combine_ref(ys, host(plan.row_of), weights.numpy(), None if base is None else base.numpy())
    return host(got).astype(np.float64), want.astype(np.float32).astype(np.float64)
