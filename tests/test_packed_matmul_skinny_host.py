"""CPU-only: the skinny (split-K, m <= 32) product with a packed (k, n) matrix as far as it goes without a device.  The two C symbols
are declared once, optional, exported and in a tuple of their own; the header states the bit contract; a library without them loads,
matmul(kernel="skinny") and PackedMatmul(kernel="skinny") raise and kernel="auto" goes to the block entry; the size function is the
skinny linear's; every argument refusal comes back through the real library with no device; the emulation means one float64 product
under all three kernel names."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _StubLibrary

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mtq.h"
NEW = ("mtq_packed_matmul_skinny_workspace_bytes", "mtq_packed_matmul_skinny")
INVALID, NO_DEVICE = -1, -3
BAD = ctypes.c_size_t(-1).value


def _last():
    return hb.lib().mtq_last_error().decode()


def test_the_two_names_are_declared_once_optional_exported_and_in_their_own_tuple():
    text = HEADER.read_text(encoding="utf-8")
    for name in NEW:
        assert len(re.findall(rf"\b{name}\s*\(", text)) == 1, name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name).argtypes is not None
    assert hb.PACKED_MATMUL_SKINNY == NEW and hb.has_packed_matmul_skinny() is True
    assert hb.PACKED_MATMUL == ("mtq_pack_tiles_transposed", "mtq_unpack_tiles_transposed", "mtq_packed_matmul")
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    assert hb.lib().mtq_packed_matmul_skinny_workspace_bytes.restype is ctypes.c_size_t
    # the skinny linear entries' parameter lists, one for one
    assert hb.SIGNATURES[NEW[0]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny_workspace_bytes"][:2]
    assert hb.SIGNATURES[NEW[1]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny"][:2]
    flat = " ".join(text.replace("*", " ").split())
    assert "y equals bit for bit what mtq_packed_linear_skinny gives, at the same split" in flat      # the bit contract is in the header
    assert packed.MATMUL_KERNELS == ("block", "skinny", "auto")
    auto = packed.AUTO_MATMUL_SKINNY_MAX_M
    assert auto is None or (isinstance(auto, int) and 1 <= auto <= packed.SKINNY_MAX_M)


def _case(m=5, n=40, k=100):
    w = gen("heavy_f32", 3, (n, k))
    pt = packed.pack_transposed(w, random_map((k, n), 6))                        # the emulation needs no library
    x = to_bf16_valued(gen("normal_f32", 4, (m, k)) * 50)
    b = gen("normal_f32", 5, (n,))
    return pt, x, b


def test_a_build_without_the_two_names_still_loads_and_auto_goes_to_the_block_entry(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_matmul.argtypes is not None and stub.mtq_packed_linear_skinny.argtypes is not None   # every other symbol is bound
    assert hb.has_packed_matmul() and not hb.has_packed_matmul_skinny()
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    pt, x, _b = _case()
    xt = torch.from_numpy(x).to(torch.bfloat16)
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul_skinny_workspace_bytes and mtq_packed_matmul_skinny.*lacks"):
        packed.matmul(xt, pt, backend="hip", kernel="skinny")                   # no other kernel in its place
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul_skinny.*lacks"):
        packed.PackedMatmul(pt, backend="hip", kernel="skinny")
    calls = []
    monkeypatch.setattr(packed, "_device_data", lambda p: "data")
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")
    monkeypatch.setattr(hb, "packed_matmul", lambda *a, **kw: calls.append(("block", a[1:], sorted(kw))) or "block result")
    monkeypatch.setattr(hb, "packed_matmul_skinny", lambda *a, **kw: calls.append(("skinny",)) or "skinny result")
    for auto in (None, 32):                                                      # whatever the measured constant is
        monkeypatch.setattr(packed, "AUTO_MATMUL_SKINNY_MAX_M", auto)
        assert packed.matmul(xt, pt, backend="hip", kernel="auto") == "block result"
    assert calls == [("block", ("data", "tables", 40), ["bias", "out_dtype"])] * 2


def test_auto_follows_the_constant_on_a_library_with_the_names(monkeypatch):
    pt, x, _b = _case(m=5)
    xt = torch.from_numpy(x).to(torch.bfloat16)
    calls = []
    monkeypatch.setattr(packed, "_device_data", lambda p: "data")
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")
    monkeypatch.setattr(hb, "packed_matmul", lambda *a, **kw: calls.append("block"))
    monkeypatch.setattr(hb, "packed_matmul_skinny", lambda *a, **kw: calls.append(("skinny", kw["split"], kw["workspace"])))
    for auto, want in ((None, "block"), (4, "block"), (5, ("skinny", 0, None)), (32, ("skinny", 0, None))):
        monkeypatch.setattr(packed, "AUTO_MATMUL_SKINNY_MAX_M", auto)
        packed.matmul(xt, pt, backend="hip", kernel="auto")
        assert calls.pop() == want, auto
    packed.matmul(xt, pt, backend="hip")                                         # the default stays the block kernel
    assert calls.pop() == "block"
    packed.matmul(xt, pt, backend="hip", kernel="skinny", split=3, workspace="ws")
    assert calls.pop() == ("skinny", 3, "ws")
    with pytest.raises(hb.MtqError, match='kernel="skinny" takes m <= 32, got m = 33'):
        packed.matmul(torch.zeros((33, 100), dtype=torch.bfloat16), pt, backend="hip", kernel="skinny")
    assert not calls


def test_the_size_function_is_the_skinny_linears():
    f, g = hb.packed_matmul_skinny_workspace_bytes, hb.packed_linear_skinny_workspace_bytes
    for m in (1, 5, 32):
        for n, k in ((1, 1), (40, 100), (72, 300), (200, 2100), (72, 4200), (19200, 512), (4096, 4096), (14336, 4096), (4096, 14336)):
            tiles_kh = -(-k // 32)
            for split in (0, 1, 2, 5, tiles_kh, tiles_kh + 3):                   # the library's choice, and a split above the tile rows
                assert f(m, n, k, split) == g(m, n, k, split), (m, n, k, split)
            assert f(m, n, k, 1) == 0 and f(m, n, k, tiles_kh + 3) == f(m, n, k, tiles_kh)
            eff = min(5, tiles_kh)
            assert f(m, n, k, 5) == (0 if eff == 1 else (eff * m * n * 4 + 15) // 16 * 16)
    assert f(32, 72, 300) == f(32, 72, 300, 2) and f(1, 72, 2100) == f(1, 72, 2100, 16) and f(1, 72, 4200) == f(1, 72, 4200, 33)
    assert f(1, 19200, 512) == f(1, 19200, 512, 3)                               # 2048 units over 600 tile columns
    L = hb.lib()
    for bad in ((0, 64, 64, 0), (33, 64, 64, 0), (1, 0, 64, 0), (1, 64, 0, 0), (1, 64, 64, -1), (1, (1 << 30) + 1, 64, 0)):
        assert int(L.mtq_packed_matmul_skinny_workspace_bytes(*bad)) == BAD, bad
        with pytest.raises(hb.MtqError):
            f(*bad)


def test_every_argument_error_needs_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    # x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, split, workspace, workspace_bytes, stream
    ok = (p, 3, 64, 64, p, big, p, p, 96, None, p, 1, 96, 2, p, big, None)       # P̂'s grid 2 x 3: at least 6 * 320 bytes

    def skinny(**kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_packed_matmul_skinny(*args)

    def refused(match, **kw):
        assert skinny(**kw) == INVALID, kw
        assert match in _last(), _last()

    for null in (0, 4, 6, 7, 10):                            # the checks of the block entry
        refused("null argument", **{f"a{null}": None})
    refused("out_dtype", a11=5)
    refused("m must be positive", a1=0)
    refused("m must be positive", a1=-2)
    refused("rows and cols must be positive", a2=0)
    refused("rows and cols must be positive", a8=0)
    refused("ldx < k", a3=63)
    refused("ldy < n", a12=95)
    refused("matrix too large", a8=(1 << 30) + 1, a12=1 << 31)
    refused("matrix too large", a2=(1 << 30) + 1, a3=1 << 31)
    refused("too many tiles", a2=1 << 30, a3=1 << 30, a8=1 << 30, a12=1 << 30)
    refused("packed must be 16-byte aligned", a4=p + 8)
    refused("smaller than the stream", a5=6 * 320 - 1)
    refused("m > 32", a1=33)                                 # and the skinny entry's own
    refused("split must not be negative", a13=-1)
    need = int(L.mtq_packed_matmul_skinny_workspace_bytes(3, 96, 64, 2))
    assert need >= 2 * 3 * 96 * 4
    refused("workspace is null", a14=None)
    refused("workspace must be 16-byte aligned", a14=p + 4)
    refused("workspace_bytes", a15=need - 1)
    refused("smaller than", a15=0)
    if not torch.cuda.is_available():                        # everything in order: only the device is missing
        assert skinny() == NO_DEVICE and skinny(a15=need) == NO_DEVICE and skinny(a11=0, a9=p) == NO_DEVICE
        assert skinny(a13=1, a14=None, a15=0) == NO_DEVICE   # split 1 needs no workspace
        assert skinny(a13=9) == NO_DEVICE                    # a split above the 2 tile rows acts as 2: the same workspace will do
        assert skinny(a5=6 * 320) == NO_DEVICE


def test_the_emulation_computes_one_product_under_the_three_names():
    pt, x, b = _case()
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.matmul(x, pt, kernel="nonsense")
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.matmul(x, pt, backend="hip", kernel="wide")                      # refused before the backend is looked at
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.PackedMatmul(pt, kernel="nonsense")
    want = packed.matmul(x, pt, bias=b)
    for kernel in packed.MATMUL_KERNELS:
        assert np.array_equal(packed.matmul(x, pt, bias=b, kernel=kernel, split=3), want), kernel
        yb = packed.matmul(x, pt, bias=b, kernel=kernel, out_dtype="bfloat16")
        assert torch.equal(yb, torch.from_numpy(want).to(torch.bfloat16))
        mod = packed.PackedMatmul(pt, bias=b, kernel=kernel)
        assert mod.backend == "emulation" and mod.kernel == kernel and mod._workspace is None and f"kernel={kernel!r}" in mod.extra_repr()
        assert np.array_equal(mod(torch.from_numpy(x).to(torch.bfloat16)).numpy(), want)
    assert packed.PackedMatmul(pt).kernel == "block"
    pt, x, b = _case(m=40)                                   # the emulation has no m limit under any name
    assert np.array_equal(packed.matmul(x, pt, bias=b, kernel="skinny"), packed.matmul(x, pt, bias=b))
