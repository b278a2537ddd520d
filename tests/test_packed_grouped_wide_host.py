"""CPU-only: the grouped wide packed linear (mtq_packed_linear_wide_grouped) as far as it goes without a device: its workspace-size
function, the entry's refusals, the bound on the row-block slots the launch covers, packed.linear_grouped_wide on the emulation and on a
library without the symbol, and PackedExperts(wide_min_rows=None), which is today's module."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _StubLibrary

WIDE = ("mtq_packed_linear_wide_grouped_workspace_bytes", "mtq_packed_linear_wide_grouped")
COUNT, N, K = 5, 72, 100
ROWS = [0, 3, 3, 131, 132, 150]


def _experts(count=COUNT, n=N, k=K, seed=0):
    w = np.stack([gen("heavy_f32", seed + 40 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((n, k), seed + 60 + i) for i in range(count)])
    return packed.pack_batch(w, maps)


def _x(rows, k=K, seed=7):
    return to_bf16_valued(gen("normal_f32", seed, (rows, k)) * 8)


def test_the_two_symbols_are_optional_exports_of_the_same_version():
    for name in WIDE:
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
    chunked = hb.SIGNATURES["mtq_packed_linear_skinny_grouped_chunked"][1]
    at = chunked.index("ilipzp") + 2                        # ... out_dtype, ldy, SPLIT, workspace, workspace_bytes, stream
    assert chunked[at] == "i" and hb.SIGNATURES[WIDE[1]][:2] == ("i", chunked[:at] + chunked[at + 1:])      # the chunked entry's, minus the split
    assert hb.SIGNATURES[WIDE[0]][:2] == ("z", "llll")
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143
    assert hb.has_packed_linear_wide_grouped()


def test_the_workspace_is_the_plan_region_and_depends_on_count_only():
    size = hb.packed_linear_wide_grouped_workspace_bytes
    shapes = [(1, 72, 300), (70, 72, 300), (200, 72, 300), (7, 40, 2100), (512, 2048, 7168), (4, 7168, 2048), (3, 5, 300), (33, 32, 64)]
    for count, want in ((1, 16), (5, 32), (300, 1216)):
        assert want == ((count + 1) * 4 + 15) // 16 * 16
        for T, n, k in shapes:
            assert size(T, count, n, k) == want, (count, T, n, k)
    raw = hb._entry(WIDE[0])
    T, count, n, k = 70, 5, 72, 300
    for bad in ((0, count, n, k), (T, 0, n, k), (T, count, 0, k), (T, count, n, 0), (-3, count, n, k), (2 ** 31, count, n, k)):
        assert raw(*bad) == 2 ** 64 - 1, bad
    with pytest.raises(hb.MtqError, match="count must be positive"):
        size(T, 0, n, k)


def test_wide_grouped_entry_checks_its_arguments_before_a_device():
    fn = hb._entry(WIDE[1])
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    T, count, n, k = 8, 2, 40, 70                           # 2 x 3 tiles each: at least 12 * 320 bytes
    need = 16
    assert hb.packed_linear_wide_grouped_workspace_bytes(T, count, n, k) == need

    def call(x=p, T=T, k=k, ldx=k, rows=p, packed_=p, nbytes=12 * 320, maps=p, offs=p, bases=p, count=count, n=n, bias=None, ldb=n, y=p, dtype=hb.DTYPE_F32,
             ldy=n, ws=p, ws_bytes=1 << 15):
        return fn(x, T, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, bias, ldb, y, dtype, ldy, ws, ws_bytes, None)

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
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bias=p, ldb=n - 1)
    refused("16-byte aligned", packed_=p + 8)
    refused("smaller than the streams", nbytes=12 * 320 - 1)
    refused("workspace is null", ws=None, ws_bytes=0)
    refused("workspace is null", ws=None, ws_bytes=1 << 15)
    refused("workspace must be 16-byte aligned", ws=p + 4)
    refused("smaller than the", ws_bytes=need - 1)
    refused("smaller than the", ws_bytes=0)


def _blocks(rows):
    return sum(-(-(b - a) // 128) for a, b in zip(rows, rows[1:]))


def _slots(T, count):
    return (T + 127 * min(count, T)) // 128


def test_the_slot_bound_holds_for_nondecreasing_rows_and_is_met():
    """The launch covers floor((T + 127 min(count, T)) / 128) row-block slots, from (T, count) alone; every block of disjoint groups has
    one: a group with rows adds at most 127/128 of a block over its rows / 128, at most min(count, T) groups have rows, and the sum of
    the block counts is an integer."""
    assert _blocks([0, 129, 258, 387]) == 6 == _slots(387, 3)                                    # equality: three groups of 128 + 1
    assert _blocks([0, 3, 3, 131, 132, 390]) == 6 and _slots(390, 5) == 8                        # surplus slots
    assert _blocks([0, 0, 300, 300, 300, 300]) == 3 <= _slots(300, 5) == 7
    assert _blocks([0, 0, 0, 1, 1, 1]) == 1 == _slots(1, 5)
    rng = np.random.default_rng(20)
    for _ in range(2000):
        count, T = int(rng.integers(1, 40)), int(rng.integers(1, 1600))
        cuts = np.sort(rng.integers(0, T + 1, size=count - 1)) if rng.random() < 0.7 else np.sort(rng.choice([0, T, T // 2], size=count - 1))
        rows = [0, *cuts.tolist(), T]
        assert _blocks(rows) <= _slots(T, count), rows
    for T in range(1, 70):                                   # every row its own group: T blocks in T slots
        assert _blocks(list(range(T + 1))) == T == _slots(T, T) == _slots(T, T + 5)


def test_the_emulation_of_linear_grouped_wide_is_linear_grouped():
    pts = _experts()
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))
    for b in (None, bias):
        want = packed.linear_grouped(x, ROWS, pts, bias=b)
        got = packed.linear_grouped_wide(x, ROWS, pts, bias=b)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(packed.linear_grouped_wide(x, ROWS, packed.batch_of(pts), bias=b, backend="emulation").view(np.uint32), want.view(np.uint32))
        assert torch.equal(packed.linear_grouped_wide(x, ROWS, pts, bias=b, out_dtype="bfloat16"),
                           packed.linear_grouped(x, ROWS, pts, bias=b, out_dtype="bfloat16"))
    assert packed.linear_grouped_wide(x[:0], [0] * (COUNT + 1), pts).shape == (0, N)
    for bad in ([0, 3, 3, 131, 132], [0, 3, 3, 131, 132, 149], [1, 3, 3, 131, 132, 150], [0, 3, 2, 131, 132, 150]):     # linear_grouped's host checks
        with pytest.raises(hb.MtqError, match="group_rows"):
            packed.linear_grouped_wide(x, bad, pts)
        with pytest.raises(hb.MtqError, match="group_rows"):
            packed.linear_grouped_wide(torch.from_numpy(x).to(torch.bfloat16), bad, pts, backend="hip")
    with pytest.raises(hb.MtqError, match="out_dtype"):
        packed.linear_grouped_wide(x, ROWS, pts, out_dtype="float16")
    with pytest.raises(hb.MtqError, match="backend"):
        packed.linear_grouped_wide(x, ROWS, pts, backend="cuda")
    assert packed.GROUPED_KERNELS == ("walk", "chunks", "auto") and packed.KERNELS == ("block", "skinny", "auto")      # a function, no fourth name


def test_without_the_symbol_the_hip_call_is_an_error_and_no_other_kernel_runs(monkeypatch):
    """Refused before any device work: this runs without a GPU, on a host batch asked onto the hip backend."""
    pts = _experts(count=2)
    monkeypatch.setattr(hb, "has_packed_linear_wide_grouped", lambda: False)

    def never(*a, **kw):
        raise AssertionError("another binding ran in place of the missing kernel")

    for name in ("packed_linear_skinny_grouped", "packed_linear_skinny_grouped_chunked", "packed_linear_wide", "packed_linear",
                 "packed_linear_wide_grouped"):
        monkeypatch.setattr(hb, name, never)
    monkeypatch.setattr(packed, "batch_to_device", never)
    x = torch.from_numpy(_x(4)).to(torch.bfloat16)
    with pytest.raises(hb.MtqError, match="mtq_packed_linear_wide_grouped.*lacks"):
        packed.linear_grouped_wide(x, [0, 2, 4], pts, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_linear_wide_grouped.*lacks"):
        packed.PackedExperts(pts, backend="hip", wide_min_rows=64)


def test_a_build_without_the_two_symbols_still_loads(monkeypatch):
    stub = _StubLibrary(143, missing=WIDE)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_linear_skinny_grouped_chunked.argtypes is not None  # every other symbol is bound
    assert not hb.has_packed_linear_wide_grouped()
    for name in WIDE:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    with pytest.raises(hb.MtqError, match="rebuild"):
        hb.packed_linear_wide_grouped_workspace_bytes(70, 5, 72, 300)


def test_packed_experts_without_wide_min_rows_is_todays_module(monkeypatch):
    pts = _experts()
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))

    def never(*a, **kw):
        raise AssertionError("forward took the wide route without a threshold")

    want = packed.linear_grouped(x, ROWS, pts, bias=bias)
    for kw in ({}, {"wide_min_rows": None}):
        mod = packed.PackedExperts(pts, bias=bias, **kw)
        assert mod.wide_min_rows is None and mod._workspace is None
        assert mod.extra_repr() == f"count={COUNT}, in_features={K}, out_features={N}, bias=True, backend='emulation', split=0"
        with monkeypatch.context() as mp:
            mp.setattr(packed, "linear_grouped_wide", never)
            assert np.array_equal(mod(torch.from_numpy(x), ROWS).numpy().view(np.uint32), want.view(np.uint32))
    assert packed.PackedExperts(pts, kernel="chunks").extra_repr().endswith("split=0, kernel='chunks'")
    # with a threshold: the emulation's product on both sides of it, and the threshold in the repr
    mod = packed.PackedExperts(pts, bias=bias, wide_min_rows=64)
    assert mod.extra_repr().endswith("split=0, wide_min_rows=64")
    assert np.array_equal(mod(torch.from_numpy(x), ROWS).numpy().view(np.uint32), want.view(np.uint32))
    small = packed.linear_grouped(x[:5], [0, 1, 1, 3, 4, 5], pts, bias=bias)
    assert np.array_equal(mod(torch.from_numpy(x[:5]), [0, 1, 1, 3, 4, 5]).numpy().view(np.uint32), small.view(np.uint32))
    for bad in (-1, 2.5, "64", True):
        with pytest.raises(hb.MtqError, match="wide_min_rows"):
            packed.PackedExperts(pts, wide_min_rows=bad)
