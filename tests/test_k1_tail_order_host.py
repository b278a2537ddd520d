"""The one property the bf16 stats kernel's tail-class redo relies on (csrc/mtq_fast.hip): inside a shared-exponent group with E in
[80, 180] the MAIN-class terms (elements within 14 binades of the maximum) of Σx, Σx² and Σ|x−y| are integer multiples of one unit with
partial sums far below 2^53 units, so their float64 sum is the same bit pattern in ANY order — the kernel may reduce them across lanes.
(The leading float32 steps of that reduce are pinned too: 4 elements of Σx, 16 of Σ|x−y| for bfp8 / bfp4 and 8 for bfp2 stay exact.)"""
import numpy as np

from oracle import mtq_oracle as orc

FORMATS = ("bfp8", "bfp4", "bfp2")   # m = 7, 3, 1
PERMS = 200


def _bf16(x):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _random_groups(rng, n):
    """n groups of 16 bf16 values: maximum exponent E in [80, 180], the others 0..20 binades below, random mantissas and signs"""
    E = rng.integers(80, 181, size=(n, 1))
    d = rng.integers(0, 21, size=(n, 16))
    d[np.arange(n), rng.integers(0, 16, size=n)] = 0
    man = rng.integers(0, 128, size=(n, 16))
    sign = rng.integers(0, 2, size=(n, 16))
    bits = (sign.astype(np.uint32) << 31) | ((E - d).astype(np.uint32) << 23) | (man.astype(np.uint32) << 16)
    return bits.view(np.float32)


def _extreme_groups():
    out = []
    for E in (80, 127, 180):
        P = np.float32(2.0) ** np.float32(E - 127)
        top, low = np.float32(1.9921875) * P, np.float32(1.9921875) * P * np.float32(2.0 ** -14)
        out.append(np.array([top] + [low] * 15, dtype=np.float32))                         # a 2P - ulp maximum, fifteen elements at d = 14
        out.append(np.array([low] * 7 + [-top] + [-low] * 8, dtype=np.float32))
        out.append(np.full(16, top, dtype=np.float32))                                     # all elements equal
        out.append(np.full(16, -np.float32(1.5) * P, dtype=np.float32))
        out.append(np.array([top, -top] * 8, dtype=np.float32))                            # alternating signs
        out.append(np.array([np.float32(1.25) * P, -low] * 8, dtype=np.float32))
    return np.stack(out)


def _seq_sum(terms):
    """float64 sum in index order along the last axis (np.add.accumulate adds one element after the other)"""
    return np.add.accumulate(terms.astype(np.float64), axis=-1)[..., -1]


def _main_terms(groups):
    """{name: [n, 16] float32 terms} with the tail-class elements' terms replaced by +0 (they are summed apart)"""
    x = _bf16(groups)
    assert np.array_equal(x, groups)
    e = (np.abs(x).view(np.uint32) >> 23).astype(np.int64)
    main = (e.max(axis=1, keepdims=True) - e) <= 14
    terms = {"x": np.where(main, x, np.float32(0)), "x2": np.where(main, x * x, np.float32(0))}
    for f in FORMATS:
        y = orc.quantize_np(x, f)
        terms["d_" + f] = np.where(main, np.abs(x - y), np.float32(0))
    return terms


def test_main_class_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(20261018)
    groups = np.concatenate([_random_groups(rng, 96), _extreme_groups()])
    perms = np.stack([rng.permutation(16) for _ in range(PERMS)])
    for name, t in _main_terms(groups).items():
        assert t.dtype == np.float32
        want = _seq_sum(t)                                                  # the contract's order
        got = _seq_sum(t[:, perms])                                         # [n, PERMS]
        assert np.array_equal(got.view(np.uint64), np.broadcast_to(want[:, None], got.shape).view(np.uint64)), name
        # a balanced tree over the 16 lanes (what the DPP row steps do) is one more order
        tree = t.astype(np.float64)
        for step in (1, 2, 4, 8):
            tree = tree[:, 0::2] + tree[:, 1::2]
        assert np.array_equal(tree[:, 0].view(np.uint64), want.view(np.uint64)), name


def test_leading_float32_steps_are_exact():
    rng = np.random.default_rng(7)
    groups = np.concatenate([_random_groups(rng, 96), _extreme_groups()])
    t = _main_terms(groups)

    def tree32(a, steps):
        for _ in range(steps):
            a = (a[:, 0::2] + a[:, 1::2]).astype(np.float32)
        return a

    def tree64(a, steps):
        a = a.astype(np.float64)
        for _ in range(steps):
            a = a[:, 0::2] + a[:, 1::2]
        return a

    for name, steps in (("x", 2), ("d_bfp8", 4), ("d_bfp4", 4), ("d_bfp2", 3)):
        for perm in (np.arange(16), np.concatenate([rng.permutation(8), 8 + rng.permutation(8)])):
            a = t[name][:, perm]
            assert np.array_equal(tree32(a, steps).astype(np.float64), tree64(a, steps)), name
