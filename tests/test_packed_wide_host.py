"""CPU-only: the wide-block packed linear's surface.  The C symbol is declared, optional and bound; every argument refusal of
mtq_packed_linear comes back from mtq_packed_linear_wide through the real library with no device; packed.linear_wide on the emulation
is packed.linear and refuses what it refuses; and kernel="auto" sends exactly m >= AUTO_WIDE_MIN_M to the wide binding, whatever the
gate is (the bindings are replaced by recorders: nothing here needs a GPU)."""
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

NAME = "mtq_packed_linear_wide"
HEADER = Path(__file__).resolve().parents[1] / "include" / "mtq.h"


def test_the_symbol_is_declared_optional_and_bound():
    text = HEADER.read_text(encoding="utf-8")
    block = re.search(r"int mtq_packed_linear\((.*?)\);", text, re.S).group(1)
    wide = re.search(r"int mtq_packed_linear_wide\((.*?)\);", text, re.S).group(1)
    assert " ".join(wide.split()) == " ".join(block.split())                # exactly the block entry's parameter list
    assert NAME in hb.SIGNATURES and NAME in hb.EXPORTS and NAME in hb.OPTIONAL_EXPORTS
    assert hb.SIGNATURES[NAME] == hb.SIGNATURES["mtq_packed_linear"]
    L = hb.lib()
    assert getattr(L, NAME).argtypes == L.mtq_packed_linear.argtypes and getattr(L, NAME).restype is ctypes.c_int
    assert hb.has_packed_linear_wide() is True
    assert L.mtq_version() == 143


def test_c_abi_argument_errors_are_the_block_entrys_and_need_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    # x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream
    ok = (p, 300, 64, 64, p, big, p, p, 64, None, p, 1, 64, None)

    def call(name, **kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        rc = getattr(L, name)(*args)
        return rc, L.mtq_last_error()

    cases = [{f"a{null}": None} for null in (0, 4, 6, 7, 10)]
    cases += [{"a11": 5}, {"a11": -1}, {"a1": 0}, {"a1": -3}, {"a2": 0}, {"a8": 0}, {"a8": -1}, {"a3": 63}, {"a12": 63}, {"a1": (1 << 40) + 1},
              {"a8": (1 << 30) + 1, "a12": 1 << 31}, {"a2": (1 << 30) + 1, "a3": 1 << 31}, {"a4": p + 8}, {"a5": 4 * 320 - 1}, {"a5": 0},
              {"a1": 1 << 40, "a8": 1 << 20, "a12": 1 << 20, "a5": 1 << 40}]             # too many workgroups for one launch
    for kw in cases:
        rc_block, msg_block = call("mtq_packed_linear", **kw)
        rc_wide, msg_wide = call(NAME, **kw)
        assert rc_block == -1, kw
        assert (rc_wide, msg_wide) == (rc_block, msg_block), (kw, msg_wide, msg_block)
    for key, word in (({"a0": None}, b"null"), ({"a11": 5}, b"out_dtype"), ({"a3": 63}, b"ldx < k"), ({"a12": 63}, b"ldy < n"),
                      ({"a1": 0}, b"m must be positive"), ({"a4": p + 8}, b"packed must be 16-byte aligned"),
                      ({"a5": 4 * 320 - 1}, b"smaller than the stream")):
        rc, msg = call(NAME, **key)
        assert rc == -1 and word in msg, (key, msg)
    if not torch.cuda.is_available():     # everything in order: only the device is missing, at every m and with a bias
        assert call(NAME)[0] == -3 and call(NAME, a1=1)[0] == -3 and call(NAME, a1=4096, a9=p)[0] == -3


def _case(m=40, n=70, k=100):
    w = gen("heavy_bf16", 3, (n, k))
    pt = packed.pack(w, random_map((n, k), 6))
    x = to_bf16_valued(gen("normal_bf16", 4, (m, k)) * 50)
    b = gen("normal_f32", 5, (n,))
    return pt, x, b


def test_linear_wide_on_emulation_is_linear():
    pt, x, b = _case()
    for bias in (None, b):
        want = packed.linear(x, pt, bias=bias)
        got = packed.linear_wide(x, pt, bias=bias)
        assert got.shape == (40, 70) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(packed.linear_wide(x, pt, bias=bias, backend="emulation").view(np.uint32), want.view(np.uint32))
        yb = packed.linear_wide(x, pt, bias=bias, out_dtype="bfloat16")
        wb = packed.linear(x, pt, bias=bias, out_dtype="bfloat16")
        assert yb.dtype == torch.bfloat16 and torch.equal(yb.view(torch.int16), wb.view(torch.int16))
    assert packed.linear_wide(x[:0], pt).shape == (0, 70)


def test_linear_wide_refuses_what_linear_refuses():
    pt, x, b = _case()
    pt3 = packed.pack(gen("normal_f32", 1, (2, 32, 64)), random_map((64, 64), 2))

    def message(fn, *args, **kw):
        with pytest.raises(hb.MtqError) as info:
            fn(*args, **kw)
        return str(info.value)

    for backend in (None, "emulation", "hip"):
        assert message(packed.linear_wide, x, pt3, backend=backend) == message(packed.linear, x, pt3, backend=backend)
        assert "2-D" in message(packed.linear_wide, x, pt3, backend=backend)
        assert message(packed.linear_wide, x, pt, out_dtype="float16", backend=backend) == message(packed.linear, x, pt, out_dtype="float16", backend=backend)
        assert "out_dtype must be" in message(packed.linear_wide, x, pt, out_dtype="float16", backend=backend)
    assert message(packed.linear_wide, x, pt, backend="nonsense") == message(packed.linear, x, pt, backend="nonsense")
    assert message(packed.linear_wide, x[:, :64], pt) == message(packed.linear, x[:, :64], pt)
    pt.layout = "transpose"
    assert message(packed.linear_wide, x, pt) == message(packed.linear, x, pt) and "row layout" in message(packed.linear_wide, x, pt)


def test_the_gate_is_none_or_above_the_skinny_range():
    gate = packed.AUTO_WIDE_MIN_M
    assert gate is None or (isinstance(gate, int) and gate > packed.AUTO_SKINNY_MAX_M)
    assert packed.KERNELS == ("block", "skinny", "auto")                    # the explicit call is a function, not a fourth name


def test_auto_calls_the_wide_binding_exactly_from_the_gate_on(monkeypatch):
    pt, _x, b = _case()
    calls = []

    def recorder(name):
        def record(x, data, tables, n, bias=None, out_dtype=None, **kw):
            calls.append((name, int(x.shape[0]), n, out_dtype))
            return name
        return record

    monkeypatch.setattr(hb, "packed_linear_wide", recorder("wide"))
    monkeypatch.setattr(hb, "packed_linear", recorder("block"))
    monkeypatch.setattr(hb, "packed_linear_skinny", recorder("skinny"))
    monkeypatch.setattr(packed, "_device_data", lambda t: t.data)           # no upload: the recorders touch nothing
    pt._tables = object()

    def routed(m, kernel="auto"):
        calls.clear()
        x = torch.zeros((m, 100), dtype=torch.bfloat16)
        got = packed.linear(x, pt, bias=b, out_dtype="bfloat16", backend="hip", kernel=kernel)
        assert len(calls) == 1 and calls[0] == (got, m, 70, torch.bfloat16)
        return got

    gate = packed.AUTO_WIDE_MIN_M
    if gate is None:
        assert routed(4096) == "block" and routed(1 << 16) == "block"
    else:
        assert routed(gate - 1) == ("block" if gate - 1 > packed.AUTO_SKINNY_MAX_M else "skinny")
        assert routed(gate) == "wide" and routed(gate + 1) == "wide" and routed(8 * gate) == "wide"
        # a library without the symbol: auto stays with the block kernel
        monkeypatch.setattr(hb, "has_packed_linear_wide", lambda: False)
        assert routed(gate) == "block"
        monkeypatch.setattr(hb, "has_packed_linear_wide", lambda: True)
    assert routed(packed.AUTO_SKINNY_MAX_M) == "skinny" and routed(packed.AUTO_SKINNY_MAX_M + 1) in ("block", "wide")
    # the other names never reach it
    for m in (33, 4096, 1 << 16):
        assert routed(m, kernel="block") == "block"
    # and the explicit call always does
    calls.clear()
    assert packed.linear_wide(torch.zeros((5, 100), dtype=torch.bfloat16), pt, backend="hip") == "wide" and calls == [("wide", 5, 70, torch.float32)]


def test_a_library_without_the_symbol_still_binds(monkeypatch):
    real = hb.lib()

    class Old:
        """A library of the same version that lacks the symbol."""

        def __getattr__(self, name):
            if name == NAME:
                raise AttributeError(name)
            return getattr(real, name)

    hb._bind(Old())                                                         # no refusal: the symbol is optional
    monkeypatch.setattr(hb, "_lib", Old())
    assert hb.has_packed_linear_wide() is False
    with pytest.raises(hb.MtqError, match=NAME):
        hb._entry(NAME)
    assert hb.tiles_hw(70, 100) == (3, 4) and hb.lib().mtq_version() == 143  # and serves everything else
