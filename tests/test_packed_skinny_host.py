"""CPU-only: the skinny (split-K, m <= 32) packed linear's surface.  The two C symbols are declared and bound, every argument refusal
the entry adds comes back through the real library with no device, the workspace size function behaves, packed.linear's `kernel`
argument is checked and means nothing to the emulation, and PackedLinear on the emulation backend is packed.linear on the flatten."""
import ctypes

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map

NAMES = ("mtq_packed_linear_skinny_workspace_bytes", "mtq_packed_linear_skinny", "mtq_debug_packed_decode")
BAD = ctypes.c_size_t(-1).value


def test_the_two_symbols_are_declared_and_bound():
    L = hb.lib()
    for name in NAMES:
        assert name in hb.SIGNATURES and hb.SIGNATURES[name][2] is True and name in hb.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.mtq_packed_linear_skinny_workspace_bytes.restype is ctypes.c_size_t
    assert hb.PACKED_SKINNY_MAX_M == packed.SKINNY_MAX_M == 32
    assert L.mtq_version() == 143


def test_c_abi_argument_errors_need_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    # x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, split, workspace, workspace_bytes, stream
    ok = (p, 3, 64, 64, p, big, p, p, 64, None, p, 1, 64, 2, p, big, None)

    def skinny(**kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_packed_linear_skinny(*args)

    # the checks of the block entry
    for null in (0, 4, 6, 7, 10):
        assert skinny(**{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert skinny(a11=5) == -1 and b"out_dtype" in L.mtq_last_error()
    assert skinny(a3=63) == -1 and b"ldx < k" in L.mtq_last_error()
    assert skinny(a12=63) == -1 and b"ldy < n" in L.mtq_last_error()
    assert skinny(a1=0) == -1 and skinny(a2=0) == -1 and skinny(a8=0) == -1
    assert skinny(a5=4 * 320 - 1) == -1 and b"smaller than the stream" in L.mtq_last_error()
    assert skinny(a4=p + 8) == -1 and b"packed must be 16-byte aligned" in L.mtq_last_error()
    # and its own
    assert skinny(a1=33) == -1 and b"m > 32" in L.mtq_last_error()
    assert skinny(a13=-1) == -1 and b"split must not be negative" in L.mtq_last_error()
    need = int(L.mtq_packed_linear_skinny_workspace_bytes(3, 64, 64, 2))
    assert need >= 2 * 3 * 64 * 4
    assert skinny(a14=None) == -1 and b"workspace is null" in L.mtq_last_error()
    assert skinny(a14=p + 4) == -1 and b"workspace must be 16-byte aligned" in L.mtq_last_error()
    assert skinny(a15=need - 1) == -1 and b"smaller than" in L.mtq_last_error() and b"workspace_bytes" in L.mtq_last_error()
    assert skinny(a15=0) == -1
    if not torch.cuda.is_available():     # everything in order: only the device is missing
        assert skinny() == -3 and skinny(a15=need) == -3
        assert skinny(a13=1, a14=None, a15=0) == -3         # split 1 needs no workspace
        assert skinny(a13=9) == -3                          # a split above tiles_w (2) acts as tiles_w: the same workspace will do


def test_decode_probe_argument_errors_need_no_device():
    L = hb.lib()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert L.mtq_debug_packed_decode(1, None, p, None) == -1 and b"null" in L.mtq_last_error()
    assert L.mtq_debug_packed_decode(1, p, None, None) == -1 and b"null" in L.mtq_last_error()
    for fmt in (0, 4, -1):
        assert L.mtq_debug_packed_decode(fmt, p, p, None) == -1 and b"fmt must be" in L.mtq_last_error()
    if not torch.cuda.is_available():
        assert L.mtq_debug_packed_decode(2, p, p, None) == -3


def test_workspace_size_function():
    f = hb.packed_linear_skinny_workspace_bytes
    for m, n, k in ((1, 64, 64), (5, 70, 160), (32, 4096, 4096), (16, 14336, 4096)):
        tiles_w = -(-k // 32)
        assert f(m, n, k, 1) == 0
        for split in (2, 5, 9, 1000):
            eff = min(split, tiles_w)
            got = f(m, n, k, split)
            assert got >= eff * m * n * 4 and got % 16 == 0 and got < eff * m * n * 4 + 16, (m, n, k, split)
            assert got == f(m, n, k, eff)
        auto = f(m, n, k)                                   # the library's choice: some split between 1 and tiles_w
        assert auto == 0 or any(auto == f(m, n, k, s) for s in range(2, tiles_w + 1)), (m, n, k)
    for n, k in ((70, 160), (4096, 4096)):
        for split in (0, 2, 5):
            sizes = [f(m, n, k, split) for m in range(1, 33)]
            assert sizes == sorted(sizes), (n, k, split)    # monotone in m: a workspace for m = 32 serves every m
    L = hb.lib()
    for bad in ((0, 64, 64, 0), (33, 64, 64, 0), (1, 0, 64, 0), (1, 64, 0, 0), (1, 64, 64, -1)):
        assert int(L.mtq_packed_linear_skinny_workspace_bytes(*bad)) == BAD, bad
        with pytest.raises(hb.MtqError):
            f(*bad)


def _case(m=5, n=70, k=100):
    w = gen("heavy_bf16", 3, (n, k))
    pt = packed.pack(w, random_map((n, k), 6))
    x = to_bf16_valued(gen("normal_bf16", 4, (m, k)) * 50)
    b = gen("normal_f32", 5, (n,))
    return pt, x, b


def test_an_unknown_kernel_is_refused_and_emulation_ignores_the_name():
    pt, x, b = _case()
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.linear(x, pt, kernel="nonsense")
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.linear(x, pt, backend="hip", kernel="nonsense")          # refused before the backend is looked at
    assert packed.KERNELS == ("block", "skinny", "auto") and 1 <= packed.AUTO_SKINNY_MAX_M <= packed.SKINNY_MAX_M
    want = packed.linear(x, pt, bias=b)
    for kernel in packed.KERNELS:
        assert np.array_equal(packed.linear(x, pt, bias=b, kernel=kernel), want), kernel
        yb = packed.linear(x, pt, bias=b, kernel=kernel, out_dtype="bfloat16")
        assert torch.equal(yb, torch.from_numpy(want).to(torch.bfloat16))
    # the emulation has no m limit under any name
    pt, x, b = _case(m=40)
    assert np.array_equal(packed.linear(x, pt, bias=b, kernel="skinny"), packed.linear(x, pt, bias=b))


def test_packed_linear_module_on_emulation():
    pt, x, b = _case(m=6)
    xt = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(xt.float(), torch.from_numpy(x))
    for bias in (None, b, torch.from_numpy(b)):
        for out_dtype in ("float32", "bfloat16"):
            layer = packed.PackedLinear(pt, bias=bias, out_dtype=out_dtype)
            assert isinstance(layer, torch.nn.Module) and layer.backend == "emulation" and layer.kernel == "auto"
            assert (layer.in_features, layer.out_features) == (100, 70) and not list(layer.parameters())
            y = layer(xt.reshape(2, 3, 100))
            want = packed.linear(x, pt, bias=None if bias is None else b, out_dtype=out_dtype)
            want = want if isinstance(want, torch.Tensor) else torch.from_numpy(want)
            assert tuple(y.shape) == (2, 3, 70) and y.dtype == want.dtype and not y.requires_grad
            assert torch.equal(y.reshape(6, 70), want)
            assert tuple(layer(xt[0]).shape) == (70,) and torch.equal(layer(xt[0]), want[0])
            assert tuple(layer(xt[:0]).shape) == (0, 70)
    assert "inference only" in packed.PackedLinear.__doc__.lower()
    with pytest.raises(hb.MtqError, match=r"\(\.\.\., 100\)"):
        packed.PackedLinear(pt)(xt[:, :64])
    with pytest.raises(hb.MtqError, match="kernel must be one of"):
        packed.PackedLinear(pt, kernel="nonsense")
    with pytest.raises(hb.MtqError, match="2-D"):
        packed.PackedLinear(packed.pack(gen("normal_f32", 1, (2, 32, 64)), random_map((64, 64), 2)))
