"""CPU-only: the grouped packed linear on the emulation backend (packed.linear_grouped / linear_batch / as_batch / PackedExperts), the host
checks of group_rows, and the grouped workspace-size function, which needs no device."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from quantization_analysis_amd.compression_algorithms.tile_utils import flatten_2d
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map

COUNT, N, K = 5, 72, 100
ROWS = [0, 32, 32, 66, 67, 70]          # groups of exactly 32, 0, 34 (above 32), 1 and 3 rows


def _experts(count=COUNT, n=N, k=K, seed=0):
    w = np.stack([gen("heavy_f32", seed + 40 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), seed + 60 + i) for i in range(count)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]
    return w, maps


def _x(rows, k=K, seed=7):
    return to_bf16_valued(gen("normal_f32", seed, (rows, k)) * 8)


def test_grouped_emulation_is_the_per_expert_linear_on_each_groups_rows():
    w, maps = _experts()
    pts = packed.pack_batch(w, maps)
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))
    for b in (None, bias):
        y = packed.linear_grouped(x, ROWS, pts, bias=b)
        assert y.shape == (ROWS[-1], N) and y.dtype == np.float32
        covered = np.zeros(ROWS[-1], dtype=bool)
        for e in range(COUNT):
            r0, r1 = ROWS[e], ROWS[e + 1]
            if r1 == r0:
                continue                                    # the empty group leaves no rows
            want = packed.linear(x[r0:r1], pts[e], bias=None if b is None else b[e])
            assert np.array_equal(y[r0:r1].view(np.uint32), want.view(np.uint32)), e
            covered[r0:r1] = True
        assert covered.all()
    # the same through a NumPy array, the batch itself being refused without its tensors on the host
    assert np.array_equal(packed.linear_grouped(x, np.asarray(ROWS), pts), packed.linear_grouped(x, ROWS, pts))
    half = packed.linear_grouped(x, ROWS, pts, out_dtype="bfloat16")
    assert half.dtype == torch.bfloat16 and torch.equal(half, torch.from_numpy(packed.linear_grouped(x, ROWS, pts)).to(torch.bfloat16))
    assert packed.linear_grouped(x[:0], [0] * (COUNT + 1), pts).shape == (0, N)      # no rows at all


def test_clamp_group_rows_is_the_kernels_rule():
    """The rule the emulation applies to a device group_rows (tests/test_packed_grouped_gpu.py runs that branch against the kernel): a host
    array always covers every row, so rows of no group exist only there."""
    T = 70
    for rows, want in (([0, 3, 3, 35, 36, 70], [(0, 3), (3, 3), (3, 35), (35, 36), (36, 70)]),
                       ([0, 3, 3, 35, 20, 20], [(0, 3), (3, 3), (3, 35), (35, 35), (20, 20)]),
                       ([0, 3, 3, 35, 36, 79], [(0, 3), (3, 3), (3, 35), (35, 36), (36, 70)]),
                       ([-5, 3, 3, 35, 36, 70], [(0, 3), (3, 3), (3, 35), (35, 36), (36, 70)]),
                       ([90, 80, -2, 2 ** 31 - 1, -2 ** 31, 5], [(70, 70), (70, 70), (0, 70), (70, 70), (0, 5)])):
        r0, r1 = packed.clamp_group_rows(np.asarray(rows, dtype=np.int32), T)
        assert list(zip(r0.tolist(), r1.tolist())) == want, rows
        assert np.all((0 <= r0) & (r0 <= r1) & (r1 <= T))


def test_linear_batch_is_linear_grouped_with_uniform_rows():
    w, maps = _experts(count=3)
    pts = packed.pack_batch(w, maps)
    m = 4
    x3 = _x(3 * m).reshape(3, m, K)
    bias = gen("normal_f32", 10, (3, N))
    y = packed.linear_batch(x3, pts, bias=bias)
    assert y.shape == (3, m, N)
    want = packed.linear_grouped(x3.reshape(3 * m, K), [0, m, 2 * m, 3 * m], pts, bias=bias)
    assert np.array_equal(y.reshape(3 * m, N).view(np.uint32), want.view(np.uint32))
    for e in range(3):
        assert np.array_equal(y[e].view(np.uint32), packed.linear(x3[e], pts[e], bias=bias[e]).view(np.uint32))
    with pytest.raises(hb.MtqError, match="x3d"):
        packed.linear_batch(x3[:2], pts)


def test_as_batch_of_a_loaded_directory_is_pack_batchs_arena(tmp_path):
    w, maps = _experts()
    pts = packed.pack_batch(w, maps)
    batch = packed.batch_of(pts)
    assert packed.as_batch(pts) is batch                    # a whole batch in order: the same object
    packed.save_dir(tmp_path / "experts", {f"layer.expert{i}.w": pt for i, pt in enumerate(pts)})
    loaded = list(packed.load_dir(tmp_path / "experts").values())
    assert packed.batch_of(loaded) is None
    again = packed.as_batch(loaded)
    assert again is not batch and again.count == COUNT and (again.rows, again.cols) == (N, K)
    assert again.arena.dtype == np.uint8 and np.array_equal(again.arena, batch.arena)
    assert again.bases.dtype == np.uint64 and np.array_equal(again.bases, batch.bases)
    x = _x(ROWS[-1])
    assert np.array_equal(packed.linear_grouped(x, ROWS, loaded).view(np.uint32), packed.linear_grouped(x, ROWS, pts).view(np.uint32))
    # a part of a batch, or another order, is built anew
    part = packed.as_batch(pts[1:3])
    assert part is not batch and part.count == 2 and np.array_equal(part.arena, np.concatenate([pts[1].data, pts[2].data]))


def test_as_batch_refuses_what_has_no_arena():
    w, maps = _experts(count=2)
    pts = packed.pack_batch(w, maps)
    other = packed.pack(gen("normal_f32", 1, (N, K + 32)), random_map((N, K + 32), 1))
    with pytest.raises(hb.MtqError, match="one 2-D shape"):
        packed.as_batch([pts[0], other])
    v = gen("normal_f32", 2, (100,))                        # a 1-D tensor
    with pytest.raises(hb.MtqError, match="2-D"):
        packed.as_batch([packed.pack(v, random_map(flatten_2d(v)[0].shape, 2))])
    with pytest.raises(hb.MtqError, match="at least one"):
        packed.as_batch([])
    pts[1].layout = "transpose"
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.as_batch(pts)
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.linear_grouped(_x(4), [0, 2, 4], pts)


def test_host_group_rows_are_checked():
    w, maps = _experts(count=3)
    pts = packed.pack_batch(w, maps)
    x = _x(10)
    packed.linear_grouped(x, [0, 4, 4, 10], pts)
    for rows, what in (([0, 6, 4, 10], "decrease"), ([0, 4, 10], "entries"), ([0, 2, 4, 8, 10], "entries"), ([1, 4, 4, 10], "start at 0"),
                       ([0, 4, 4, 9], "end at"), ([0, 4, 4, 11], "end at"), ([[0, 4], [4, 10]], "entries"), ([0.0, 4.0, 4.0, 10.0], "integers")):
        with pytest.raises(hb.MtqError, match=what):
            packed.linear_grouped(x, rows, pts)
    with pytest.raises(hb.MtqError, match="x must be"):
        packed.linear_grouped(x[:, :-1], [0, 4, 4, 10], pts)
    with pytest.raises(hb.MtqError, match="bias"):
        packed.linear_grouped(x, [0, 4, 4, 10], pts, bias=np.zeros((2, N), dtype=np.float32))
    with pytest.raises(hb.MtqError, match="out_dtype"):
        packed.linear_grouped(x, [0, 4, 4, 10], pts, out_dtype="float16")


def test_packed_experts_on_the_emulation():
    w, maps = _experts()
    pts = packed.pack_batch(w, maps)
    bias = gen("normal_f32", 11, (COUNT, N))
    mod = packed.PackedExperts(pts, bias=bias)
    assert mod.backend == "emulation" and (mod.count, mod.out_features, mod.in_features) == (COUNT, N, K)
    x = _x(ROWS[-1])
    y = mod(torch.from_numpy(x), ROWS)
    assert np.array_equal(y.numpy().view(np.uint32), packed.linear_grouped(x, ROWS, pts, bias=bias).view(np.uint32))
    none = mod(torch.from_numpy(x[:0]), [0] * (COUNT + 1))
    assert tuple(none.shape) == (0, N)
    with pytest.raises(hb.MtqError, match="bias"):
        packed.PackedExperts(pts, bias=bias[:2])


def test_grouped_workspace_bytes_needs_no_device():
    f = hb.packed_linear_skinny_grouped_workspace_bytes
    T, count, n, k = 70, 5, 72, 300                         # 10 tile columns
    assert f(T, count, n, k, 1) == 0
    for split, eff in ((2, 2), (3, 3), (10, 10), (13, 10)):  # a split above tiles_w acts as tiles_w
        assert f(T, count, n, k, split) == (eff * T * n * 4 + 15) // 16 * 16
    assert f(3, 2, 5, 300, 3) == (3 * 3 * 5 * 4 + 15) // 16 * 16 == 192      # rounded up to 16
    own = f(T, count, n, k, 0)
    assert own % (T * n * 4) == 0 and 1 <= own // (T * n * 4) <= 10
    for m, n1, k1 in ((1, 4096, 4096), (32, 4096, 4096), (4, 2048, 7168), (4, 7168, 2048), (7, 72, 300), (3, 40, 2100)):
        assert f(m, 1, n1, k1, 0) == hb.packed_linear_skinny_workspace_bytes(m, n1, k1, 0), (m, n1, k1)
    # more experts never ask for more slices than one does
    assert f(4, 256, 2048, 7168, 0) <= f(4, 1, 2048, 7168, 0)
    raw = hb._entry("mtq_packed_linear_skinny_grouped_workspace_bytes")
    assert raw(T, count, n, k, -1) == 2 ** 64 - 1
    assert raw(0, count, n, k, 1) == 2 ** 64 - 1 and raw(T, 0, n, k, 1) == 2 ** 64 - 1 and raw(T, count, 0, k, 1) == 2 ** 64 - 1
    with pytest.raises(hb.MtqError, match="split must not be negative"):
        f(T, count, n, k, -1)


def test_grouped_entry_checks_its_arguments_before_a_device():
    fn = hb._entry("mtq_packed_linear_skinny_grouped")
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    T, count, n, k = 8, 2, 40, 70                           # 2 x 3 tiles each: at least 12 * 320 bytes

    def call(x=p, T=T, k=k, ldx=k, rows=p, packed_=p, nbytes=12 * 320, maps=p, offs=p, bases=p, count=count, n=n, bias=None, ldb=n, y=p, dtype=hb.DTYPE_F32,
             ldy=n, split=1, ws=None, ws_bytes=0):
        return fn(x, T, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, bias, ldb, y, dtype, ldy, split, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == -1
        assert match in hb.lib().mtq_last_error().decode(), hb.lib().mtq_last_error().decode()

    for name in ("x", "rows", "packed_", "maps", "offs", "bases", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=7)
    refused("total_rows must be positive", T=0)
    refused("32-bit group_rows", T=2 ** 31)
    refused("count must be positive", count=0)
    refused("count does not fit 32 bits", count=2 ** 31)
    refused("rows and cols must be positive", n=0)
    refused("split must not be negative", split=-1)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bias=p, ldb=n - 1)
    refused("16-byte aligned", packed_=p + 8)
    refused("smaller than the streams", nbytes=12 * 320 - 1)
    refused("workspace is null", split=2)
    refused("workspace must be 16-byte aligned", split=2, ws=p + 4, ws_bytes=1 << 15)
    refused("smaller than the", split=2, ws=p, ws_bytes=2 * T * n * 4 - 16)
