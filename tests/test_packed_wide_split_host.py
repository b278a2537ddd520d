"""CPU-only: include/mtq_wide_split.h against WIDE_SPLIT_SIGNATURES, the split rule and the size functions of the wide split entries, what
the C entries refuse without a device, and how packed.linear_wide / matmul_wide route `split` (recorders in place of the bindings)."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb, packed
from tests.packed_cases import _grid_case, random_map

LETTER = {"int": "i", "int64_t": "l", "size_t": "z"}
LINEAR, MATMUL = "mtq_packed_linear_wide_split", "mtq_packed_matmul_wide_split"


def test_header_is_the_signature_table_and_the_names_are_optional():
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).parents[1] / "include" / "mtq_wide_split.h").read_text(), flags=re.S)
    found = {}
    for result, name, params in re.findall(r"^(int|size_t) (mtq_\w+)\(([^;]*)\);", text, flags=re.M):
        kinds = ["p" if "*" in p else LETTER[p.split()[0]] for p in params.replace("\n", " ").split(",")]
        found[name] = (LETTER[result], "".join(kinds), True)
    assert found == hb.WIDE_SPLIT_SIGNATURES and hb.WIDE_SPLIT_EXPORTS == tuple(found) and hb.packed_wide_split_available()
    assert not set(found) & set(hb.EXPORTS) and hb.lib().mtq_version() == 143


@pytest.mark.parametrize("m,n,k", ((40, 96, 200), (300, 130, 64), (1, 1, 4096)))
def test_split_rule_and_sizes(m, n, k):
    steps = -(-k // 64)
    for split, want in ((1, 1), (2, min(2, steps)), (steps, steps), (steps + 1, steps)):
        assert hb.packed_wide_split(m, n, k, split) == want
        size = 0 if want == 1 else (want * m * n * 4 + 15) // 16 * 16
        assert hb.packed_linear_wide_split_workspace(m, n, k, split) == hb.packed_matmul_wide_split_workspace(m, n, k, split) == size
    auto = hb.packed_wide_split(m, n, k, 0)
    assert 1 <= auto <= steps and auto == hb.packed_wide_split(m, n, k, 0)
    for bad in (dict(split=-1), dict(m=0), dict(n=0), dict(k=0)):
        args = {**dict(m=m, n=n, k=k, split=1), **bad}
        assert hb.lib().mtq_packed_wide_split(*args.values()) == -1
        with pytest.raises(hb.MtqError):
            hb.packed_linear_wide_split_workspace(*args.values())
    # blocks alone fill the chip: the library's choice is 1
    assert hb.packed_wide_split(4096, 4096, 4096, 0) == 1 and hb.packed_wide_split(64, 4096, 4096, 0) > 1


@pytest.mark.parametrize("name,wide", ((LINEAR, "mtq_packed_linear_wide"), (MATMUL, "mtq_packed_matmul_wide")))
def test_c_abi_refusals_without_a_device(name, wide):
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    need = 2 * 300 * 96 * 4
    # x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy | split, workspace, workspace_bytes | stream
    ok = (p, 300, 200, 200, p, 1 << 20, p, p, 96, None, p, 1, 96, 2, p, need, None)

    def call(entry, **kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        if entry == wide:
            del args[13:16]
        return getattr(L, entry)(*args), L.mtq_last_error()

    cases = [{f"a{null}": None} for null in (0, 4, 6, 7, 10)]
    cases += [{"a11": 5}, {"a1": 0}, {"a2": 0}, {"a8": -1}, {"a3": 199}, {"a12": 95}, {"a1": (1 << 40) + 1}, {"a4": p + 8}, {"a5": 21 * 320 - 1},
              {"a1": 1 << 40, "a8": 1 << 20, "a12": 1 << 20, "a5": 1 << 40}]
    for kw in cases:
        got, want = call(name, **kw), call(wide, **kw)
        assert want[0] == -1 and got == want, (kw, got, want)
    for kw, word in (({"a13": -1}, b"split must not be negative"), ({"a14": None}, b"workspace is null"), ({"a14": p + 4}, b"workspace must be"),
                     ({"a15": need - 1}, b"workspace_bytes"), ({"a13": 5, "a15": 4 * 300 * 96 * 4 - 1}, b"workspace_bytes")):
        rc, msg = call(name, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    if not torch.cuda.is_available():     # everything in order: only the device is missing; an effective split of 1 wants no workspace
        assert call(name)[0] == -3 and call(name, a13=0, a15=1 << 30)[0] == -3 and call(name, a13=5, a15=4 * 300 * 96 * 4)[0] == -3
        assert call(name, a13=1, a14=None, a15=0)[0] == -3 and call(name, a2=64, a3=64, a5=1 << 20, a14=None, a15=0)[0] == -3


def _pair(m=40, n=70, k=200):
    x, w, b = _grid_case(m, n, k, 5)
    return x, b, packed.pack(w, random_map((n, k), 3)), packed.pack(np.ascontiguousarray(w.T), random_map((k, n), 4))


@pytest.mark.parametrize("which", ("linear", "matmul"))
def test_split_1_is_the_old_binding_and_any_other_the_new_one(monkeypatch, which):
    _x, _b, nk, kn = _pair()
    pt, fn = (nk, packed.linear_wide) if which == "linear" else (kn, packed.matmul_wide)
    calls = []
    monkeypatch.setattr(packed, "_device_data", lambda p: "data")
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")
    for name in (f"packed_{which}_wide", f"packed_{which}_wide_split"):
        monkeypatch.setattr(hb, name, lambda x, data, tables, n, name=name, **kw: calls.append((name, n, kw)) or torch.zeros((int(x.shape[0]), n)))
    xb = torch.zeros((40, 200), dtype=torch.bfloat16)
    fn(xb, pt, backend="hip")
    fn(xb, pt, backend="hip", split=1, workspace="ws")
    assert calls == [(f"packed_{which}_wide", 70, dict(bias=None, out_dtype=torch.float32))] * 2       # today's call, keyword for keyword
    calls.clear()
    for split in (0, 2, 7):
        fn(xb, pt, backend="hip", split=split, workspace="ws", out_dtype="bfloat16")
    assert calls == [(f"packed_{which}_wide_split", 70, dict(bias=None, out_dtype=torch.bfloat16, split=s, workspace="ws")) for s in (0, 2, 7)]
    for bad in (-1, 1.5, True):
        with pytest.raises(hb.MtqError, match="split must be"):
            fn(xb, pt, backend="hip", split=bad)
    mod = (packed.PackedLinear if which == "linear" else packed.PackedMatmul)
    assert "wide_split" not in mod(pt, backend="emulation").extra_repr() and "wide_split=0" in mod(pt, backend="emulation", wide_split=0).extra_repr()
    # a library without the new names: the explicit split raises naming them, split 1 still reaches the old binding
    monkeypatch.setattr(hb, "lib", lambda: types.SimpleNamespace(**{f"mtq_packed_{w}_wide": 1 for w in ("linear", "matmul")},
                                                                  **{n: 1 for n in hb.PACKED_MATMUL}))
    calls.clear()
    with pytest.raises(hb.MtqError, match=f"{LINEAR} and {MATMUL}, which this build of libmtq_hip.so lacks"):
        fn(xb, pt, backend="hip", split=0)
    with pytest.raises(hb.MtqError, match="lacks"):
        mod(pt, backend="hip", wide_split=2)
    fn(xb, pt, backend="hip")
    assert [c[0] for c in calls] == [f"packed_{which}_wide"]


def test_the_emulation_gives_the_same_bits_at_every_split():
    x, b, nk, kn = _pair()
    for pt, fn, mod in ((nk, packed.linear_wide, packed.PackedLinear), (kn, packed.matmul_wide, packed.PackedMatmul)):
        want = fn(x, pt, bias=b)
        for split in (0, 2, 3, 9):
            assert np.array_equal(fn(x, pt, bias=b, split=split, backend="emulation").view(np.uint32), want.view(np.uint32))
        got = mod(pt, bias=b, backend="emulation", wide_split=0)(torch.from_numpy(x).to(torch.bfloat16))
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
