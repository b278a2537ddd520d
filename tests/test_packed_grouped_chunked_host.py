"""CPU-only: the chunked grouped packed linear (mtq_packed_linear_skinny_grouped_chunked) as far as it goes without a device: its
workspace-size function against the walking entry's, the entry's refusals, the bound on the chunk slots the launch covers, and the
`kernel=` of packed.linear_grouped / linear_batch / PackedExperts on the emulation."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _StubLibrary

CHUNKED = ("mtq_packed_linear_skinny_grouped_chunked_workspace_bytes", "mtq_packed_linear_skinny_grouped_chunked")
COUNT, N, K = 5, 72, 100
ROWS = [0, 32, 32, 66, 67, 70]


def _experts(count=COUNT, n=N, k=K, seed=0):
    w = np.stack([gen("heavy_f32", seed + 40 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), seed + 60 + i) for i in range(count)])
    return packed.pack_batch(w, maps)


def _x(rows, k=K, seed=7):
    return to_bf16_valued(gen("normal_f32", seed, (rows, k)) * 8)


def test_the_two_symbols_are_optional_exports_of_the_same_version():
    for name in CHUNKED:
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS
    assert hb.SIGNATURES[CHUNKED[0]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny_grouped_workspace_bytes"][:2]
    assert hb.SIGNATURES[CHUNKED[1]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny_grouped"][:2]      # the same parameters in the same order
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143
    assert hb.has_packed_linear_grouped_chunked()


def test_the_plan_region_depends_on_count_only():
    """chunked − walking is the plan region: (count + 1) int32 rounded up to 16, whatever (T, n, k, split) is — so the two entries'
    effective splits, which the walking entry's bytes encode, are equal, split 0 included."""
    chunked, walking = hb.packed_linear_skinny_grouped_chunked_workspace_bytes, hb.packed_linear_skinny_grouped_workspace_bytes
    shapes = [(1, 72, 300), (70, 72, 300), (200, 72, 300), (7, 40, 2100), (512, 2048, 7168), (4, 7168, 2048), (3, 5, 300), (33, 32, 64)]
    for count in (1, 5, 300):
        plan = ((count + 1) * 4 + 15) // 16 * 16
        for T, n, k in shapes:
            for split in (0, 1, 2, 4, 13, 1000):
                c, w = chunked(T, count, n, k, split), walking(T, count, n, k, split)
                assert c - w == plan and c % 16 == 0 and c > 0, (count, T, n, k, split, c, w)
    assert chunked(70, 5, 72, 300, 1) == 32                  # never 0: split 1 still holds the plan
    raw = hb._entry(CHUNKED[0])
    T, count, n, k = 70, 5, 72, 300
    for bad in ((0, count, n, k, 1), (T, 0, n, k, 1), (T, count, 0, k, 1), (T, count, n, 0, 1), (T, count, n, k, -1), (-3, count, n, k, 1)):
        assert raw(*bad) == 2 ** 64 - 1, bad
    with pytest.raises(hb.MtqError, match="split must not be negative"):
        chunked(T, count, n, k, -1)


def test_chunked_entry_checks_its_arguments_before_a_device():
    fn = hb._entry(CHUNKED[1])
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    T, count, n, k = 8, 2, 40, 70                           # 2 x 3 tiles each: at least 12 * 320 bytes
    need1, need2 = 16, 16 + 2 * T * n * 4
    assert hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, 1) == need1
    assert hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, 2) == need2

    def call(x=p, T=T, k=k, ldx=k, rows=p, packed_=p, nbytes=12 * 320, maps=p, offs=p, bases=p, count=count, n=n, bias=None, ldb=n, y=p, dtype=hb.DTYPE_F32,
             ldy=n, split=1, ws=p, ws_bytes=1 << 15):
        return fn(x, T, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, bias, ldb, y, dtype, ldy, split, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == -1
        assert match in hb.lib().mtq_last_error().decode(), hb.lib().mtq_last_error().decode()

    for name in ("x", "rows", "packed_", "maps", "offs", "bases", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=7)
    refused("total_rows must be positive", T=0)
    refused("total_rows must be positive", T=-1)
    refused("32-bit group_rows", T=2 ** 31)
    refused("count must be positive", count=0)
    refused("count must be positive", count=-2)
    refused("count does not fit 32 bits", count=2 ** 31)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", n=-1, ldy=0)
    refused("rows and cols must be positive", k=0, ldx=0)
    refused("rows and cols must be positive", k=-1, ldx=0)
    refused("split must not be negative", split=-1)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bias=p, ldb=n - 1)
    refused("16-byte aligned", packed_=p + 8)
    refused("smaller than the streams", nbytes=12 * 320 - 1)
    for split, need in ((1, need1), (2, need2), (0, hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, 0))):
        refused("workspace is null", split=split, ws=None, ws_bytes=0)       # at split 1 too: the plan lives there
        refused("workspace is null", split=split, ws=None, ws_bytes=1 << 15)
        refused("workspace must be 16-byte aligned", split=split, ws=p + 4)
        refused("smaller than the", split=split, ws_bytes=need - 1)
        refused("smaller than the", split=split, ws_bytes=0)


def _chunks(rows):
    return sum(-(-(b - a) // 32) for a, b in zip(rows, rows[1:]))


def _slots(T, count):
    return (T + 31 * min(count, T)) // 32


def test_the_slot_bound_holds_for_nondecreasing_rows_and_is_met():
    """The launch covers floor((T + 31 min(count, T)) / 32) chunk slots, from (T, count) alone; every chunk of disjoint groups has one."""
    assert _chunks([0, 33, 66, 99]) == 6 == _slots(99, 3)                                        # equality: three groups of 32 + 1
    assert _chunks([0, 0, 130, 131, 200, 200]) == 9 and _slots(200, 5) == 11                     # surplus slots
    assert _chunks([0, 0, 0, 1, 1, 1]) == 1 == _slots(1, 5)
    assert _chunks([0, 3, 3, 35, 36, 70]) == 5 <= _slots(70, 5) == 7
    rng = np.random.default_rng(20)
    for _ in range(2000):
        count, T = int(rng.integers(1, 40)), int(rng.integers(1, 400))
        cuts = np.sort(rng.integers(0, T + 1, size=count - 1)) if rng.random() < 0.7 else np.sort(rng.choice([0, T, T // 2], size=count - 1))
        rows = [0, *cuts.tolist(), T]
        assert _chunks(rows) <= _slots(T, count), rows
    for T in range(1, 70):                                   # every row its own group: T chunks in T slots
        assert _chunks(list(range(T + 1))) == T == _slots(T, T) == _slots(T, T + 5)


def test_every_kernel_name_is_the_same_product_on_the_emulation():
    assert packed.GROUPED_KERNELS == ("walk", "chunks", "auto") and packed.GROUPED_AUTO_KERNEL in ("walk", "chunks")
    pts = _experts()
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))
    want = packed.linear_grouped(x, ROWS, pts, bias=bias, kernel="walk")
    assert np.array_equal(want.view(np.uint32), packed.linear_grouped(x, ROWS, pts, bias=bias).view(np.uint32))      # the default
    x3 = _x(COUNT * 4).reshape(COUNT, 4, K)
    for kernel in packed.GROUPED_KERNELS:
        assert np.array_equal(packed.linear_grouped(x, ROWS, pts, bias=bias, kernel=kernel).view(np.uint32), want.view(np.uint32)), kernel
        half = packed.linear_grouped(x, ROWS, pts, out_dtype="bfloat16", kernel=kernel)
        assert torch.equal(half, packed.linear_grouped(x, ROWS, pts, out_dtype="bfloat16"))
        assert np.array_equal(packed.linear_batch(x3, pts, kernel=kernel), packed.linear_batch(x3, pts)), kernel
        mod = packed.PackedExperts(pts, bias=bias, kernel=kernel)
        assert mod.backend == "emulation" and mod.kernel == (packed.GROUPED_AUTO_KERNEL if kernel == "auto" else kernel)
        assert np.array_equal(mod(torch.from_numpy(x), ROWS).numpy().view(np.uint32), want.view(np.uint32)), kernel


def test_an_unknown_kernel_name_is_refused():
    pts = _experts(count=2)
    x = _x(4)
    for name in ("skinny", "chunk", "", None):
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.linear_grouped(x, [0, 2, 4], pts, kernel=name)
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.linear_batch(x.reshape(2, 2, K), pts, kernel=name)
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.PackedExperts(pts, kernel=name)


def test_chunks_without_the_symbol_is_an_error_not_the_other_kernel(monkeypatch):
    """Refused before any device work: this runs without a GPU, on a host batch asked onto the hip backend."""
    pts = _experts(count=2)
    monkeypatch.setattr(hb, "has_packed_linear_grouped_chunked", lambda: False)

    def never(*a, **kw):
        raise AssertionError("the walking entry ran in place of the missing kernel")

    monkeypatch.setattr(hb, "packed_linear_skinny_grouped", never)
    monkeypatch.setattr(packed, "batch_to_device", never)
    x = torch.from_numpy(_x(4)).to(torch.bfloat16)
    with pytest.raises(hb.MtqError, match="chunks.*lacks"):
        packed.linear_grouped(x, [0, 2, 4], pts, backend="hip", kernel="chunks")
    with pytest.raises(hb.MtqError, match="chunks.*lacks"):
        packed.linear_batch(x.reshape(2, 2, K), pts, backend="hip", kernel="chunks")
    with pytest.raises(hb.MtqError, match="chunks.*lacks"):
        packed.PackedExperts(pts, backend="hip", kernel="chunks")
    monkeypatch.setattr(packed, "GROUPED_AUTO_KERNEL", "chunks")
    with pytest.raises(hb.MtqError, match="chunks.*lacks"):
        packed.linear_grouped(x, [0, 2, 4], pts, backend="hip", kernel="auto")


def test_a_build_without_the_two_symbols_still_loads(monkeypatch):
    stub = _StubLibrary(143, missing=CHUNKED)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_linear_skinny_grouped.argtypes is not None          # every other symbol is bound
    assert not hb.has_packed_linear_grouped_chunked()
    for name in CHUNKED:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    with pytest.raises(hb.MtqError, match="rebuild"):
        hb.packed_linear_skinny_grouped_chunked_workspace_bytes(70, 5, 72, 300, 1)
