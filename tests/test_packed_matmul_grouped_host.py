"""CPU-only: the grouped packed matmul for (k, n) experts (mtq_packed_matmul_skinny_grouped, _chunked and mtq_packed_matmul_wide_grouped)
as far as it goes without a device: the emulation contract of packed.matmul_grouped / matmul_batch / matmul_grouped_wide, their refusals,
the six optional symbols and their size functions against the grouped linear ones, the entries' argument checks (nothing is launched), and
a library without the symbols."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _OnDevice, _StubLibrary

WALK = ("mtq_packed_matmul_skinny_grouped_workspace_bytes", "mtq_packed_matmul_skinny_grouped")
CHUNKED = ("mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes", "mtq_packed_matmul_skinny_grouped_chunked")
WIDE = ("mtq_packed_matmul_wide_grouped_workspace_bytes", "mtq_packed_matmul_wide_grouped")
SIX = WALK + CHUNKED + WIDE
COUNT, N, K = 5, 72, 100                                    # non-square: k x n experts, 4 x 3 tiles
ROWS = [0, 3, 3, 35, 36, 70]


def _experts(count=COUNT, n=N, k=K, seed=0):
    """`count` (k, n) experts from (n, k) weights, through pack_batch_transposed's emulation, and the weights."""
    w = np.stack([gen("heavy_f32", seed + 40 + i, (n, k)) for i in range(count)])
    maps = np.stack([random_map((k, n), seed + 60 + i) for i in range(count)])
    return packed.pack_batch_transposed(w, maps), w, maps


def _x(rows, k=K, seed=7):
    return to_bf16_valued(gen("normal_f32", seed, (rows, k)) * 8)


def _words(a):
    return a.view(np.uint32) if isinstance(a, np.ndarray) else a.view(torch.int16)


# ----------------------------------------------------------------------------- the emulation contract

def test_the_emulation_is_matmul_per_group_and_rows_of_no_group_are_zeros():
    pts, _w, _maps = _experts()
    assert (pts[0].rows, pts[0].cols) == (K, N)
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))
    for b in (None, bias):
        want = np.zeros((ROWS[-1], N), dtype=np.float32)
        for e in range(COUNT):
            r0, r1 = ROWS[e], ROWS[e + 1]
            want[r0:r1] = packed.matmul(x[r0:r1], pts[e], bias=None if b is None else b[e], backend="emulation")
        for kernel in packed.MATMUL_GROUPED_KERNELS:           # the same product under every kernel name
            got = packed.matmul_grouped(x, ROWS, pts, bias=b, backend="emulation", kernel=kernel)
            assert got.dtype == np.float32 and np.array_equal(_words(got), _words(want)), kernel
            half = packed.matmul_grouped(x, ROWS, pts, bias=b, out_dtype="bfloat16", kernel=kernel)
            assert torch.equal(half, torch.from_numpy(want).to(torch.bfloat16))
        wide = packed.matmul_grouped_wide(x, ROWS, packed.batch_of(pts), bias=b, backend="emulation")
        assert np.array_equal(_words(wide), _words(want))
    # rows of no group are zeros: what the emulation makes of a device group_rows (clamp_group_rows) leaves rows 35.. to no group
    # (a host group_rows must cover every row; tests/test_packed_matmul_grouped_gpu.py hands the emulation the device array itself)
    r0, r1 = packed.clamp_group_rows([0, 3, 3, 35, 20, 20], ROWS[-1])
    assert list(zip(r0.tolist(), r1.tolist())) == [(0, 3), (3, 3), (3, 35), (35, 35), (20, 20)]
    none = packed.matmul_grouped(x, [0] * COUNT + [ROWS[-1]], pts[:COUNT - 1] + [pts[0]], bias=None)      # the last expert takes every row
    assert np.array_equal(_words(none), _words(packed.matmul(x, pts[0], backend="emulation")))
    assert packed.matmul_grouped(x[:0], [0] * (COUNT + 1), pts).shape == (0, N)
    assert packed.matmul_grouped_wide(x[:0], [0] * (COUNT + 1), pts).shape == (0, N)
    assert packed.MATMUL_GROUPED_KERNELS == ("walk", "chunks", "auto") and packed.MATMUL_GROUPED_AUTO_KERNEL in ("walk", "chunks")


def test_matmul_batch_is_the_grouped_call_with_equal_groups():
    pts, _w, _maps = _experts()
    m = 4
    x3 = _x(COUNT * m).reshape(COUNT, m, K)
    bias = gen("normal_f32", 9, (COUNT, N))
    y = packed.matmul_batch(x3, pts, bias=bias)
    assert y.shape == (COUNT, m, N)
    for e in range(COUNT):
        assert np.array_equal(_words(np.ascontiguousarray(y[e])), _words(packed.matmul(x3[e], pts[e], bias=bias[e], backend="emulation")))
    with pytest.raises(hb.MtqError, match="x3d must be"):
        packed.matmul_batch(_x(COUNT * m, N).reshape(COUNT, m, N), pts)


def test_an_input_major_batch_and_a_transposed_batch_give_the_same_product():
    """pack_batch of the (k, n) matrices Wᵀ under the same maps is the same arena: the batch forms the docstring names are one format."""
    pts, w, maps = _experts()
    direct = packed.pack_batch(np.ascontiguousarray(w.transpose(0, 2, 1)), maps)
    x = _x(ROWS[-1])
    assert np.array_equal(_words(packed.matmul_grouped(x, ROWS, direct)), _words(packed.matmul_grouped(x, ROWS, pts)))
    loaded = [packed.PackedTensor(pt.shape, pt.shape_info, pt.rows, pt.cols, pt.map, pt.offsets, np.array(pt.data[: pt.nbytes])) for pt in pts]
    assert packed.batch_of(loaded) is None                  # as_batch concatenates this list
    assert np.array_equal(_words(packed.matmul_grouped(x, ROWS, loaded)), _words(packed.matmul_grouped(x, ROWS, pts)))


def test_refusals():
    pts, _w, _maps = _experts()
    x = _x(ROWS[-1])
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.matmul_grouped(x, ROWS, pts, kernel="block")
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.PackedExpertsMatmul(pts, kernel="wide")
    for fn in (packed.matmul_grouped, packed.matmul_grouped_wide):
        with pytest.raises(hb.MtqError, match=rf"x must be \(T, {K}\)"):                          # n instead of k: the orientation
            fn(_x(ROWS[-1], N), ROWS, pts)
        with pytest.raises(hb.MtqError, match=rf"x must be \(T, {K}\)"):
            fn(torch.from_numpy(_x(ROWS[-1], N)).to(torch.bfloat16), ROWS, pts, backend="hip")
        with pytest.raises(hb.MtqError, match=rf"bias must be \({COUNT}, {N}\)"):
            fn(x, ROWS, pts, bias=np.zeros((COUNT, K), dtype=np.float32))
        for bad in ([0, 3, 3, 35, 36], [0, 3, 3, 35, 36, 69], [1, 3, 3, 35, 36, 70], [0, 3, 2, 35, 36, 70]):
            with pytest.raises(hb.MtqError, match="group_rows"):
                fn(x, bad, pts)
            with pytest.raises(hb.MtqError, match="group_rows"):
                fn(torch.from_numpy(x).to(torch.bfloat16), bad, pts, backend="hip")
        with pytest.raises(hb.MtqError, match="out_dtype"):
            fn(x, ROWS, pts, out_dtype="float16")
        with pytest.raises(hb.MtqError, match="backend"):
            fn(x, ROWS, pts, backend="cuda")
    other, _w2, _m2 = _experts(count=1, n=N + 32)
    with pytest.raises(hb.MtqError, match="one 2-D shape"):
        packed.matmul_grouped(x, [0, 3, 70], [pts[0], other[0]])
    with pytest.raises(hb.MtqError, match=rf"bias must be \({COUNT}, {N}\)"):
        packed.PackedExpertsMatmul(pts, bias=np.zeros((COUNT, K), dtype=np.float32))


def test_the_module_on_the_emulation():
    pts, _w, _maps = _experts()
    x = _x(ROWS[-1])
    bias = gen("normal_f32", 9, (COUNT, N))
    want = packed.matmul_grouped(x, ROWS, pts, bias=bias)
    for kw in ({}, {"kernel": "chunks"}, {"wide_min_rows": 64}, {"wide_min_rows": 71}):
        mod = packed.PackedExpertsMatmul(pts, bias=bias, **kw)
        assert (mod.count, mod.in_features, mod.out_features) == (COUNT, K, N) and mod.backend == "emulation" and mod._workspace is None
        assert np.array_equal(_words(mod(torch.from_numpy(x), ROWS).numpy()), _words(want))
    assert packed.PackedExpertsMatmul(pts).extra_repr() == f"count={COUNT}, in_features={K}, out_features={N}, bias=False, backend='emulation', split=0"
    assert packed.PackedExpertsMatmul(pts, kernel="chunks", wide_min_rows=64).extra_repr().endswith("split=0, kernel='chunks', wide_min_rows=64")
    for bad in (-1, 2.5, "64", True):
        with pytest.raises(hb.MtqError, match="wide_min_rows"):
            packed.PackedExpertsMatmul(pts, wide_min_rows=bad)
    with pytest.raises(hb.MtqError, match=rf"x must be \(T, {K}\)"):
        packed.PackedExpertsMatmul(pts)(torch.zeros((4, N)), [0, 1, 2, 3, 4, 4])


# ----------------------------------------------------------------------------- the C ABI

def test_the_six_symbols_are_optional_exports_of_the_same_version():
    for name in SIX:
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name, None) is not None, name                                    # exported by the built library
        assert hb.SIGNATURES[name][:2] == hb.SIGNATURES[name.replace("mtq_packed_matmul_", "mtq_packed_linear_")][:2], name
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143
    assert hb.has_packed_matmul_grouped() and hb.has_packed_matmul_grouped_chunked() and hb.has_packed_matmul_wide_grouped()


SHAPES = [(70, 5, 72, 300, s) for s in (0, 1, 2, 13)] + [
    (1, 1, 1, 1, 0), (7, 2, 40, 2100, 0), (7, 2, 40, 2100, 5), (70, 5, 300, 72, 0), (70, 5, 300, 72, 3), (256, 64, 2048, 7168, 0),
    (256, 64, 7168, 2048, 0), (40, 300, 256, 512, 0),        # count * ceil(n/32) = 2400 > 2048: the library's split is 1
    (40, 300, 256, 512, 4), (33, 3, 32, 64, 2), (1000, 9, 200, 104, 0)]


def test_the_size_functions_are_the_grouped_linear_ones():
    assert 300 * -(-256 // 32) > 2048
    for T, count, n, k, s in SHAPES:
        walk = hb.packed_matmul_skinny_grouped_workspace_bytes(T, count, n, k, s)
        assert walk == hb.packed_linear_skinny_grouped_workspace_bytes(T, count, n, k, s), (T, count, n, k, s)
        chunked = hb.packed_matmul_skinny_grouped_chunked_workspace_bytes(T, count, n, k, s)
        assert chunked == hb.packed_linear_skinny_grouped_chunked_workspace_bytes(T, count, n, k, s) > 0, (T, count, n, k, s)
        assert chunked == walk + ((count + 1) * 4 + 15) // 16 * 16
        assert hb.packed_matmul_wide_grouped_workspace_bytes(T, count, n, k) == hb.packed_linear_wide_grouped_workspace_bytes(T, count, n, k) \
            == ((count + 1) * 4 + 15) // 16 * 16
    assert hb.packed_matmul_skinny_grouped_workspace_bytes(40, 300, 256, 512, 0) == 0             # past kSkinnyUnits tile rows: no split
    assert hb.packed_matmul_skinny_grouped_workspace_bytes(70, 5, 72, 300, 13) == 10 * 70 * 72 * 4  # a split above ceil(k/32) acts as ceil(k/32)
    T, count, n, k = 70, 5, 72, 300
    for name in (WALK[0], CHUNKED[0]):
        raw = hb._entry(name)
        for bad in ((0, count, n, k, 0), (T, 0, n, k, 0), (T, count, 0, k, 0), (T, count, n, 0, 0), (T, count, n, k, -1), (2 ** 31, count, n, k, 0)):
            assert raw(*bad) == 2 ** 64 - 1, (name, bad)
    for bad in ((0, count, n, k), (T, 0, n, k), (T, count, 0, k), (T, count, n, 0)):
        assert hb._entry(WIDE[0])(*bad) == 2 ** 64 - 1, bad
    with pytest.raises(hb.MtqError, match="count must be positive"):
        hb.packed_matmul_skinny_grouped_workspace_bytes(T, 0, n, k)
    with pytest.raises(hb.MtqError, match="split must not be negative"):
        hb.packed_matmul_skinny_grouped_chunked_workspace_bytes(T, count, n, k, -1)


@pytest.mark.parametrize("names", [WALK, CHUNKED, WIDE], ids=["walk", "chunks", "wide"])
def test_the_entries_check_their_arguments_before_a_device(names):
    """Host pointers throughout: a call that got past a check would look for a device; every one of these ends before that."""
    fn = hb._entry(names[1])
    has_split = names is not WIDE
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    T, count, n, k = 8, 2, 40, 150                          # k x n: 5 x 2 tiles each, at least 20 * 320 bytes; split 2 is in effect
    need = hb._entry(names[0])(T, count, n, k, *((2,) if has_split else ()))
    assert need == {WALK: 2 * T * n * 4, CHUNKED: 16 + 2 * T * n * 4, WIDE: 16}[names]

    def call(x=p, T=T, k=k, ldx=k, rows=p, packed_=p, nbytes=20 * 320, maps=p, offs=p, bases=p, count=count, n=n, bias=None, ldb=n, y=p,
             dtype=hb.DTYPE_F32, ldy=n, split=2, ws=p, ws_bytes=1 << 15):
        return fn(x, T, k, ldx, rows, packed_, nbytes, maps, offs, bases, count, n, bias, ldb, y, dtype, ldy, *((split,) if has_split else ()), ws,
                  ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == -1
        assert match in hb.lib().mtq_last_error().decode(), hb.lib().mtq_last_error().decode()

    for name in ("x", "rows", "packed_", "maps", "offs", "bases", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=7)
    refused("total_rows must be positive", T=0)
    refused("32-bit group_rows", T=2 ** 31)
    refused("count must be positive", count=0)
    refused("count must be positive", count=-2)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", k=0, ldx=0)
    refused("ldx < k", ldx=k - 1)
    refused("ldx < k", ldx=n)                               # the contraction is k, not n
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bias=p, ldb=n - 1)
    refused("16-byte aligned", packed_=p + 8)
    refused("smaller than the streams", nbytes=20 * 320 - 1)
    refused("workspace is null", ws=None, ws_bytes=0)
    refused("workspace must be 16-byte aligned", ws=p + 4)
    refused("smaller than the", ws_bytes=need - 1)
    if has_split:
        refused("split must not be negative", split=-1)


def test_the_bindings_refuse_what_the_library_would_dereference():
    """Through hip_backend with null-pointer stand-ins for device tensors: a call that passed every check of the binding is refused by the
    library's own null check, never launched."""
    count, n, k, T = 2, 40, 150, 8
    tiles = 5 * 2
    x = _OnDevice(torch.zeros((T, k), dtype=torch.bfloat16))
    rows = _OnDevice(torch.zeros(count + 1, dtype=torch.int32))
    arena = _OnDevice(torch.zeros(count * tiles * 320, dtype=torch.uint8))
    maps = _OnDevice(torch.zeros((count, tiles), dtype=torch.int8))
    offs = _OnDevice(torch.zeros((count, tiles + 1), dtype=torch.int32))
    bases = _OnDevice(torch.zeros(count + 1, dtype=torch.int64))
    out = _OnDevice(torch.zeros((T, n), dtype=torch.float32))
    ws = _OnDevice(torch.zeros(1 << 14, dtype=torch.uint8))
    for fn in (hb.packed_matmul_skinny_grouped, hb.packed_matmul_skinny_grouped_chunked, hb.packed_matmul_wide_grouped):
        with pytest.raises(hb.MtqError, match="null argument"):
            fn(x, rows, arena, maps, offs, bases, count, n, out=out, workspace=ws, stream=None)
        with pytest.raises(hb.MtqError):                     # a wider x: the tables and the arena are of a smaller grid
            fn(_OnDevice(torch.zeros((T, k + 64), dtype=torch.bfloat16)), rows, arena, maps, offs, bases, count, n, out=out, workspace=ws, stream=None)
        with pytest.raises(hb.MtqError, match="bias"):
            fn(x, rows, arena, maps, offs, bases, count, n, bias=_OnDevice(torch.zeros((count, k))), out=out, workspace=ws, stream=None)
        with pytest.raises(hb.MtqError, match="group_rows"):
            fn(x, _OnDevice(torch.zeros(count, dtype=torch.int32)), arena, maps, offs, bases, count, n, out=out, workspace=ws, stream=None)


# ----------------------------------------------------------------------------- a library without the symbols

def test_without_the_symbols_the_hip_call_is_an_error_and_no_other_kernel_runs(monkeypatch):
    stub = _StubLibrary(143, missing=SIX)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_matmul_skinny.argtypes is not None and stub.mtq_packed_linear_skinny_grouped_chunked.argtypes is not None
    assert not (hb.has_packed_matmul_grouped() or hb.has_packed_matmul_grouped_chunked() or hb.has_packed_matmul_wide_grouped())
    for name in SIX:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    with pytest.raises(hb.MtqError, match="rebuild"):
        hb.packed_matmul_skinny_grouped_workspace_bytes(70, 5, 72, 300)

    def never(*a, **kw):
        raise AssertionError("another binding ran in place of the missing kernel, or device work began")

    for name in ("packed_linear_skinny_grouped", "packed_linear_skinny_grouped_chunked", "packed_linear_wide_grouped", "packed_matmul",
                 "packed_matmul_skinny", "packed_matmul_wide", "packed_matmul_skinny_grouped", "packed_matmul_skinny_grouped_chunked",
                 "packed_matmul_wide_grouped", "require_gpu"):
        monkeypatch.setattr(hb, name, never)
    monkeypatch.setattr(packed, "batch_to_device", never)
    pts, _w, _maps = _experts(count=2)
    x = torch.from_numpy(_x(4)).to(torch.bfloat16)
    for kernel, symbol in (("walk", WALK[1]), ("chunks", CHUNKED[1])):
        with pytest.raises(hb.MtqError, match=rf"{symbol} .*lacks: rebuild"):
            packed.matmul_grouped(x, [0, 2, 4], pts, backend="hip", kernel=kernel)
        with pytest.raises(hb.MtqError, match=rf"{symbol} .*lacks: rebuild"):
            packed.PackedExpertsMatmul(pts, backend="hip", kernel=kernel)
    with pytest.raises(hb.MtqError, match=rf"{WIDE[1]} .*lacks: rebuild"):
        packed.matmul_grouped_wide(x, [0, 2, 4], pts, backend="hip")
    # the wide kernel alone missing: the skinny route exists, the threshold is refused in the constructor
    only_wide = _StubLibrary(143, missing=WIDE)
    assert _load(monkeypatch, only_wide) is only_wide and hb.has_packed_matmul_grouped() and not hb.has_packed_matmul_wide_grouped()
    with pytest.raises(hb.MtqError, match=rf"{WIDE[1]} .*lacks: rebuild"):
        packed.PackedExpertsMatmul(pts, backend="hip", wide_min_rows=64)
