"""CPU-only: the wide-block product with a packed (k, n) matrix as far as it goes without a device.  The C symbol is declared once with
its bit contract, optional, exported and bound with mtq_packed_matmul's signature; a library without it loads, matmul_wide raises
naming it and matmul(kernel="auto") goes to the block entry; on a library with it "auto" follows AUTO_MATMUL_WIDE_MIN_M; every argument
refusal of mtq_packed_matmul comes back from the wide entry through the real library with no device; the emulation is matmul's."""
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
NAME = "mtq_packed_matmul_wide"


def test_the_symbol_is_declared_with_its_contract_optional_exported_and_bound():
    text = HEADER.read_text(encoding="utf-8")
    assert len(re.findall(rf"\b{NAME}\s*\(", text)) == 1
    block = re.search(r"int mtq_packed_matmul\((.*?)\);", text, re.S).group(1)
    wide = re.search(rf"int {NAME}\((.*?)\);", text, re.S).group(1)
    assert " ".join(wide.split()) == " ".join(block.split())                     # exactly mtq_packed_matmul's parameter list
    flat = " ".join(text.replace("*", " ").split())
    assert "y equals mtq_packed_matmul's bit for bit, in both output types, with and without bias" in flat
    assert NAME in hb.SIGNATURES and NAME in hb.EXPORTS and NAME in hb.OPTIONAL_EXPORTS and hb.SIGNATURES[NAME][2] is True
    assert hb.SIGNATURES[NAME] == hb.SIGNATURES["mtq_packed_matmul"]
    L = hb.lib()
    assert getattr(L, NAME).argtypes == L.mtq_packed_matmul.argtypes and getattr(L, NAME).restype is ctypes.c_int
    assert hb.has_packed_matmul_wide() is True
    assert hb.MTQ_VERSION == 143 and L.mtq_version() == 143 and packed.FORMAT_VERSION == 1
    assert packed.MATMUL_KERNELS == ("block", "skinny", "auto")                  # the explicit call is a function, not a fourth name
    gate = packed.AUTO_MATMUL_WIDE_MIN_M
    assert gate is None or (isinstance(gate, int) and gate > packed.SKINNY_MAX_M)


def _case(m=5, n=40, k=100):
    w = gen("heavy_f32", 3, (n, k))
    pt = packed.pack_transposed(w, random_map((k, n), 6))                        # the emulation needs no library
    x = to_bf16_valued(gen("normal_f32", 4, (m, k)) * 50)
    b = gen("normal_f32", 5, (n,))
    return pt, x, b


DATA = torch.zeros(1, dtype=torch.uint8)                                         # stands for the device stream: no recorder reads it


def _recorders(monkeypatch, calls):
    """The three bindings replaced by recorders of (name, m, (data, tables, n), keywords) that return an (m, n) tensor."""
    monkeypatch.setattr(packed, "_device_data", lambda p: DATA)
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")

    def recorder(name):
        def record(x, data, tables, n, **kw):
            assert data is DATA
            calls.append((name, int(x.shape[0]), (tables, n), sorted(k for k in kw if k not in ("split", "workspace"))))
            return torch.zeros((int(x.shape[0]), n))
        return record

    for name in ("block", "skinny", "wide"):
        monkeypatch.setattr(hb, "packed_matmul" + ("" if name == "block" else "_" + name), recorder(name))


def test_a_build_without_the_symbol_still_loads_raises_by_name_and_auto_goes_to_the_block_entry(monkeypatch):
    stub = _StubLibrary(143, missing=(NAME,))
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_matmul.argtypes is not None and stub.mtq_packed_matmul_skinny.argtypes is not None   # every other symbol is bound
    assert hb.has_packed_matmul() and hb.has_packed_matmul_skinny() and not hb.has_packed_matmul_wide()
    with pytest.raises(hb.MtqError, match=f"has no {NAME}.*rebuild"):
        hb._entry(NAME)
    pt, _x, _b = _case()
    x300 = torch.zeros((300, 100), dtype=torch.bfloat16)
    calls = []
    _recorders(monkeypatch, calls)
    with pytest.raises(hb.MtqError, match=f"{NAME}.*lacks"):
        packed.matmul_wide(x300, pt, backend="hip")                              # no other kernel in its place
    assert not calls
    for gate in (None, 33, 64, 300, 301):                                        # whatever the measured constant is
        monkeypatch.setattr(packed, "AUTO_MATMUL_WIDE_MIN_M", gate)
        assert tuple(packed.matmul(x300, pt, backend="hip", kernel="auto").shape) == (300, 40)
        assert tuple(packed.PackedMatmul(pt, backend="hip", kernel="auto")(x300).shape) == (300, 40)
    assert calls == [("block", 300, ("tables", 40), ["bias", "out_dtype"])] * 10


def test_auto_follows_the_constant_on_a_library_with_the_symbol(monkeypatch):
    stub = _StubLibrary(143)
    assert _load(monkeypatch, stub) is stub and hb.has_packed_matmul_wide()
    pt, _x, b = _case()
    calls = []
    _recorders(monkeypatch, calls)

    def routed(m, kernel="auto", **kw):
        calls.clear()
        got = packed.matmul(torch.zeros((m, 100), dtype=torch.bfloat16), pt, bias=b, out_dtype="bfloat16", backend="hip", kernel=kernel, **kw)
        assert len(calls) == 1 and calls[0][1:] == (m, ("tables", 40), ["bias", "out_dtype"]) and tuple(got.shape) == (m, 40)
        return calls[0][0]

    m = 300
    for gate, want in ((None, "block"), (m - 1, "wide"), (m, "wide"), (m + 1, "block")):
        monkeypatch.setattr(packed, "AUTO_MATMUL_WIDE_MIN_M", gate)
        assert routed(m) == want, gate
        skinny_max = packed.AUTO_MATMUL_SKINNY_MAX_M
        assert routed(skinny_max) == "skinny" and routed(1) == "skinny"          # the decode range stays the skinny kernel's
        assert routed(skinny_max + 1) == ("wide" if gate is not None and skinny_max + 1 >= gate else "block")
        for mm in (1, 33, m, 1 << 16):                                           # the default and the explicit name never reach it
            assert routed(mm, kernel="block") == "block"
        mod = packed.PackedMatmul(pt, bias=b, backend="hip", kernel="auto")
        calls.clear()
        assert tuple(mod(torch.zeros((2, m // 2, 100), dtype=torch.bfloat16)).shape) == (2, m // 2, 40) and calls[0][0] == want
    # a gate inside the skinny range does not take its rows away
    monkeypatch.setattr(packed, "AUTO_MATMUL_WIDE_MIN_M", 8)
    assert routed(8) == "skinny" and routed(32) == "skinny" and routed(33) == "wide"
    # and the explicit call always reaches the wide binding
    calls.clear()
    assert tuple(packed.matmul_wide(torch.zeros((5, 100), dtype=torch.bfloat16), pt, backend="hip").shape) == (5, 40)
    assert calls == [("wide", 5, ("tables", 40), ["bias", "out_dtype"])]


def test_c_abi_argument_errors_are_the_block_entrys_and_need_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    # x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream
    ok = (p, 300, 64, 64, p, big, p, p, 96, None, p, 1, 96, None)                # P̂'s grid 2 x 3: at least 6 * 320 bytes

    def call(name, **kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        rc = getattr(L, name)(*args)
        return rc, L.mtq_last_error()

    cases = [{f"a{null}": None} for null in (0, 4, 6, 7, 10)]
    cases += [{"a11": 5}, {"a11": -1}, {"a1": 0}, {"a1": -3}, {"a2": 0}, {"a8": 0}, {"a8": -1}, {"a3": 63}, {"a12": 95}, {"a1": (1 << 40) + 1},
              {"a8": (1 << 30) + 1, "a12": 1 << 31}, {"a2": (1 << 30) + 1, "a3": 1 << 31},
              {"a2": 1 << 30, "a3": 1 << 30, "a8": 1 << 30, "a12": 1 << 30}, {"a4": p + 8}, {"a5": 6 * 320 - 1}, {"a5": 0},
              {"a1": 1 << 40, "a8": 1 << 20, "a12": 1 << 20, "a5": 1 << 40}]             # too many workgroups for one launch
    for kw in cases:
        rc_block, msg_block = call("mtq_packed_matmul", **kw)
        rc_wide, msg_wide = call(NAME, **kw)
        assert rc_block == -1, kw
        assert (rc_wide, msg_wide) == (rc_block, msg_block), (kw, msg_wide, msg_block)
    for key, word in (({"a0": None}, b"null"), ({"a11": 5}, b"out_dtype"), ({"a3": 63}, b"ldx < k"), ({"a12": 95}, b"ldy < n"),
                      ({"a1": 0}, b"m must be positive"), ({"a8": 0}, b"rows and cols must be positive"),
                      ({"a4": p + 8}, b"packed must be 16-byte aligned"), ({"a5": 6 * 320 - 1}, b"smaller than the stream"),
                      ({"a1": 1 << 40, "a8": 1 << 20, "a12": 1 << 20, "a5": 1 << 40}, b"too many workgroups")):
        rc, msg = call(NAME, **key)
        assert rc == -1 and word in msg, (key, msg)
    if not torch.cuda.is_available():     # everything in order: only the device is missing, at every m and with a bias
        assert call(NAME)[0] == -3 and call(NAME, a1=1)[0] == -3 and call(NAME, a1=4096, a9=p, a11=0)[0] == -3
        assert call(NAME, a5=6 * 320)[0] == -3


def test_matmul_wide_on_the_emulation_is_matmul_and_refuses_what_it_refuses():
    pt, x, b = _case(m=40)
    for bias in (None, b):
        want = packed.matmul(x, pt, bias=bias)
        got = packed.matmul_wide(x, pt, bias=bias)
        assert got.shape == (40, 40) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(packed.matmul_wide(x, pt, bias=bias, backend="emulation").view(np.uint32), want.view(np.uint32))
        yb = packed.matmul_wide(x, pt, bias=bias, out_dtype="bfloat16")
        wb = packed.matmul(x, pt, bias=bias, out_dtype="bfloat16")
        assert yb.dtype == torch.bfloat16 and torch.equal(yb.view(torch.int16), wb.view(torch.int16))
    assert packed.matmul_wide(x[:0], pt).shape == (0, 40)

    def message(fn, *args, **kw):
        with pytest.raises(hb.MtqError) as info:
            fn(*args, **kw)
        return str(info.value)

    pt3 = packed.pack(gen("normal_f32", 1, (2, 32, 64)), random_map((64, 64), 2))
    assert "2-D" in message(packed.matmul_wide, x, pt3)
    assert message(packed.matmul_wide, x, pt, out_dtype="float16") == message(packed.matmul, x, pt, out_dtype="float16")
    assert message(packed.matmul_wide, x, pt, backend="nonsense") == message(packed.matmul, x, pt, backend="nonsense")
    assert message(packed.matmul_wide, x[:, :64], pt) == message(packed.matmul, x[:, :64], pt)
    pt.layout = "transpose"
    assert message(packed.matmul_wide, x, pt) == message(packed.matmul, x, pt) and "row layout" in message(packed.matmul_wide, x, pt)
