"""CPU-only: the fused gated product for decode (packed.glu_skinny, packed.glu_grouped_skinny, PackedMLP(decode_kernel="fused"),
PackedExpertsMLP(decode_max_rows=...)) as far as it goes without a device.  The four C symbols are declared, optional and exported; the
size functions give the header's formula and are never 0; every refusal comes back before a device is looked for (the pointers handed
in are host addresses that no check may dereference); the emulation is glu's / glu_grouped's; the modules reach the expected
bindings (replaced by recorders: nothing here needs a GPU) and their defaults reach what they reached before."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import random_map
from tests.test_capi_host import _load, _OnDevice, _StubLibrary

HEADER = Path(__file__).resolve().parents[1] / "include" / "mtq.h"
NEW = ("mtq_packed_glu_skinny_workspace_bytes", "mtq_packed_glu_skinny", "mtq_packed_glu_skinny_grouped_workspace_bytes",
       "mtq_packed_glu_skinny_grouped")
INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -3
BAD_SIZE = 2 ** 64 - 1
N, K = 40, 100


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def _round16(v):
    return (v + 15) // 16 * 16


def test_the_entries_are_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name) is not None
    assert set(hb.PACKED_GLU_SKINNY) == set(NEW) and hb.has_packed_glu_skinny() is True
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    # the wide entries' parameters, then split, workspace, workspace_bytes, the stream last
    assert hb.SIGNATURES[NEW[1]][1] == hb.SIGNATURES["mtq_packed_glu_wide"][1][:-1] + "ipzp"
    assert hb.SIGNATURES[NEW[3]][1] == hb.SIGNATURES["mtq_packed_glu_wide_grouped"][1][:-3] + "ipzp"
    assert hb.SIGNATURES[NEW[0]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny_workspace_bytes"][:2]
    assert hb.SIGNATURES[NEW[2]][:2] == hb.SIGNATURES["mtq_packed_linear_skinny_grouped_workspace_bytes"][:2]
    assert "there is no fused kernel for the decode range" not in re.sub(r"\s*\n \*\s*", " ", text)


def test_a_build_without_the_entries_still_loads_and_nothing_stands_in(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_wide_grouped.argtypes is not None                 # every other symbol is bound
    assert hb.has_packed_glu() and not hb.has_packed_glu_skinny()
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    gate = packed.pack(gen("heavy_f32", 1, (N, K)), random_map((N, K), 2))
    down = packed.pack(gen("heavy_f32", 3, (64, N)), random_map((64, N), 4))
    x = torch.zeros((4, K), dtype=torch.bfloat16)
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_skinny.*lacks.*rebuild it from this tree"):
        packed.glu_skinny(x, gate, gate, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_skinny.*lacks.*rebuild it from this tree"):
        packed.glu_grouped_skinny(x, [0, 4], [gate], [gate], backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_skinny.*lacks"):
        packed.PackedMLP(gate, gate, down, backend="hip", decode_kernel="fused")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_skinny.*lacks"):
        packed.PackedExpertsMLP([gate], [gate], [down], backend="hip", decode_max_rows=8)


def test_the_size_functions_give_the_formula_and_never_zero():
    dense = hb._entry(NEW[0])
    # (m, n, k): 40 x 100 is 2 x 4 tiles, the library's split there is max(1, min(2048 / 2, 4 / 4)) = 1; 96 x 2080 is 3 x 65: 16
    for m, n, k, own in ((5, 40, 100, 1), (32, 96, 2080, 16), (1, 32, 32, 1)):
        tiles_w = (k + 31) // 32
        for split, eff in ((0, own), (1, 1), (2, min(2, tiles_w)), (tiles_w + 7, tiles_w), (1000, tiles_w)):
            want = _round16(2 * eff * m * n * 4)
            assert hb.packed_glu_skinny_workspace_bytes(m, n, k, split) == want > 0, (m, n, k, split)
            linear = hb.packed_linear_skinny_workspace_bytes(m, n, k, split)     # the shared rule: twice the linear entry's partials
            assert linear == (0 if eff == 1 else _round16(eff * m * n * 4))
    assert hb.packed_glu_skinny_workspace_bytes(1, 33, 32, 0) == _round16(2 * 33 * 4) == 272    # rounded up to 16
    for bad in ((0, 40, 100, 0), (33, 40, 100, 0), (-1, 40, 100, 0), (5, 0, 100, 0), (5, 40, 0, 0), (5, 40, 100, -1), (5, (1 << 30) + 1, 100, 0)):
        assert dense(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.packed_glu_skinny_workspace_bytes(*bad)
    grouped = hb._entry(NEW[2])
    for T, count, n, k in ((21, 3, 40, 100), (70, 1, 96, 288), (7, 3, 40, 2100), (1, 1, 32, 32)):
        tiles_h, tiles_w = (n + 31) // 32, (k + 31) // 32
        own = max(1, min(2048 // (count * tiles_h), tiles_w // 4))
        for split, eff in ((0, own), (1, 1), (2, min(2, tiles_w)), (tiles_w + 1, tiles_w)):
            want = _round16(2 * eff * T * n * 4)
            assert hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, split) == want > 0, (T, count, n, k, split)
        if count == 1 and T <= 32:                       # one group: the dense entry's rule and size
            assert hb.packed_glu_skinny_grouped_workspace_bytes(T, 1, n, k, 0) == hb.packed_glu_skinny_workspace_bytes(T, n, k, 0)
    for bad in ((0, 3, 40, 100, 0), (2 ** 31, 3, 40, 100, 0), (21, 0, 40, 100, 0), (21, 2 ** 31, 40, 100, 0), (21, 3, 0, 100, 0), (21, 3, 40, 0, 0),
                (21, 3, 40, 100, -1), (2 ** 31 - 1, 1, 1 << 30, 32, 1)):
        assert grouped(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.packed_glu_skinny_grouped_workspace_bytes(*bad)


def test_glu_skinny_refuses_before_a_device():
    fn = hb._entry(NEW[1])
    _buf, p = _aligned()
    m, n, k = 8, 64, 64                                   # 2 x 2 tiles: at least 4 * 320 bytes a stream
    need = hb.packed_glu_skinny_workspace_bytes(m, n, k, 0)
    assert need == 2 * m * n * 4

    def call(x=p, m=m, k=k, ldx=k, gp=p, gbytes=1 << 20, gmap=p, goff=p, up=p, ubytes=1 << 20, umap=p, uoff=p, n=n, bg=None, bu=None, act=0, y=p,
             dtype=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        return fn(x, m, k, ldx, gp, gbytes, gmap, goff, up, ubytes, umap, uoff, n, bg, bu, act, y, dtype, ldy, split, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "gp", "gmap", "goff", "up", "umap", "uoff", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=5)
    refused("m must be positive", m=0)
    refused("m must be positive", m=-3)
    refused("m > 32", m=33)
    refused("split must not be negative", split=-1)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", k=0)
    refused("matrix too large", n=(1 << 30) + 1, ldy=1 << 31)
    refused("matrix too large", k=(1 << 30) + 1, ldx=1 << 31)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("packed must be 16-byte aligned", gp=p + 8)
    refused("packed must be 16-byte aligned", up=p + 8)
    refused("smaller than the stream", gbytes=4 * 320 - 1)
    refused("smaller than the stream", ubytes=4 * 320 - 1)
    refused("smaller than the stream", ubytes=0)
    for split in (0, 1, 2, 1000):                         # the workspace at every split, split 1 included
        size = hb.packed_glu_skinny_workspace_bytes(m, n, k, split)
        refused("workspace is null", split=split, ws=None, ws_bytes=0)
        refused("workspace is null", split=split, ws=None)
        refused("workspace must be 16-byte aligned", split=split, ws=p + 4)
        refused("smaller than the", split=split, ws_bytes=size - 1)
        refused("smaller than the", split=split, ws_bytes=0)
    for act in (2, -1, 7):
        assert call(act=act) == UNSUPPORTED and "act must be" in _last()
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert call() == NO_DEVICE and call(m=1, act=1, bg=p, bu=p, split=2, ws_bytes=need) == NO_DEVICE
        assert call(m=32, dtype=hb.DTYPE_BF16, split=1, ws_bytes=2 * 32 * n * 4) == NO_DEVICE


def test_glu_skinny_grouped_refuses_before_a_device():
    fn = hb._entry(NEW[3])
    _buf, p = _aligned()
    T, count, n, k = 8, 2, 40, 70                         # 2 x 3 tiles each: at least 12 * 320 bytes an arena
    need = hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, 0)
    assert need == 2 * T * n * 4

    def call(x=p, T=T, k=k, ldx=k, rows=p, gp=p, gbytes=12 * 320, gmaps=p, goffs=p, gbases=p, up=p, ubytes=12 * 320, umaps=p, uoffs=p, ubases=p,
             count=count, n=n, bg=None, bu=None, ldb=n, act=0, y=p, dtype=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
        return fn(x, T, k, ldx, rows, gp, gbytes, gmaps, goffs, gbases, up, ubytes, umaps, uoffs, ubases, count, n, bg, bu, ldb, act, y, dtype, ldy,
                  split, ws, ws_bytes, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "rows", "gp", "gmaps", "goffs", "gbases", "up", "umaps", "uoffs", "ubases", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=7)
    refused("total_rows must be positive", T=0)
    refused("total_rows must be positive", T=-1)
    refused("32-bit group_rows", T=2 ** 31)
    refused("count must be positive", count=0)
    refused("count does not fit 32 bits", count=2 ** 31)
    refused("split must not be negative", split=-2)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", k=0, ldx=0)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("ldb < n", bg=p, ldb=n - 1)
    refused("ldb < n", bu=p, ldb=n - 1)
    refused("16-byte aligned", gp=p + 8)
    refused("16-byte aligned", up=p + 8)
    refused("smaller than the streams", gbytes=12 * 320 - 1)
    refused("smaller than the streams", ubytes=12 * 320 - 1)
    refused("workspace of this split is too large", T=2 ** 31 - 1, n=1 << 30, ldy=1 << 30, k=32, ldx=32, count=1, gbytes=1 << 40, ubytes=1 << 40, split=1)
    for split in (0, 1, 2):
        size = hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, split)
        refused("workspace is null", split=split, ws=None, ws_bytes=0)
        refused("workspace must be 16-byte aligned", split=split, ws=p + 4)
        refused("smaller than the", split=split, ws_bytes=size - 1)
    for act in (2, -1):
        assert call(act=act) == UNSUPPORTED and "act must be" in _last()
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(ldb=n - 1, ws_bytes=need) == NO_DEVICE      # without a bias ldb means nothing
        assert call(split=3, dtype=hb.DTYPE_BF16, bg=p, bu=p, ws_bytes=3 * need) == NO_DEVICE


def test_the_bindings_check_their_operands_before_a_device():
    """hb.packed_glu_skinny over tensors that only claim to be on the device: what the binding refuses is refused before any pointer is
    used."""
    tables, wider = SimpleNamespace(tiles_h=2, tiles_w=4), SimpleNamespace(tiles_h=2, tiles_w=6)
    x = _OnDevice(torch.zeros((4, K), dtype=torch.bfloat16))
    with pytest.raises(hb.MtqError, match="m <= 32"):
        hb.packed_glu_skinny(_OnDevice(torch.zeros((33, K), dtype=torch.bfloat16)), None, tables, None, tables, N)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_glu_skinny(_OnDevice(torch.zeros((4, K))), None, tables, None, tables, N)
    with pytest.raises(hb.MtqError, match="the up map is 2x6 tiles"):
        hb.packed_glu_skinny(x, None, tables, None, wider, N)
    with pytest.raises(hb.MtqError, match="the gate map is 2x6 tiles"):
        hb.packed_glu_skinny(x, None, wider, None, tables, N)
    with pytest.raises(hb.MtqError, match="act must be"):
        hb.packed_glu_skinny(x, None, tables, None, tables, N, act="gelu")
    with pytest.raises(hb.MtqError, match="output type"):
        hb.packed_glu_skinny(x, None, tables, None, tables, N, out_dtype=torch.float16)


# ----------------------------------------------------------------------------- the emulation

def _pair(n=N, k=K):
    wg, wu = gen("heavy_f32", 21, (n, k)), gen("heavy_f32", 22, (n, k))
    return packed.pack(wg, random_map((n, k), 23)), packed.pack(wu, random_map((n, k), 24))


def test_the_emulation_of_glu_skinny_is_glu():
    gate, up = _pair()
    x = to_bf16_valued(gen("normal_f32", 25, (37, K)) * 4)       # the emulation takes any m
    bg, bu = gen("normal_f32", 26, (N,)), gen("normal_f32", 27, (N,))
    for b_g, b_u in ((None, None), (bg, None), (None, bu), (bg, bu)):
        for act in packed.ACTS:
            for split in (0, 1, 3):
                want = packed.glu(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u)
                got = packed.glu_skinny(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, split=split)
                assert got.dtype == np.float32 and got.shape == (37, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            wb = packed.glu(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, out_dtype="bfloat16")
            gb = packed.glu_skinny(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, out_dtype="bfloat16", backend="emulation")
            assert gb.dtype == torch.bfloat16 and torch.equal(gb.view(torch.int16), wb.view(torch.int16))
    assert packed.glu_skinny(x[:0], gate, up).shape == (0, N)
    other = packed.pack(gen("heavy_f32", 1, (N, K + 32)), random_map((N, K + 32), 2))
    for backend in (None, "emulation", "hip"):
        with pytest.raises(hb.MtqError, match="one shape"):
            packed.glu_skinny(x, gate, other, backend=backend)
        with pytest.raises(hb.MtqError, match="act must be"):
            packed.glu_skinny(x, gate, up, act="gelu", backend=backend)
        with pytest.raises(hb.MtqError, match="out_dtype"):
            packed.glu_skinny(x, gate, up, out_dtype="float16", backend=backend)
    with pytest.raises(hb.MtqError, match="backend must be"):
        packed.glu_skinny(x, gate, up, backend="cuda")


def _experts(count=3, k_out=64):
    wg = np.stack([gen("heavy_f32", 30 + i, (N, K)) for i in range(count)])
    wu = np.stack([gen("heavy_f32", 40 + i, (N, K)) for i in range(count)])
    wd = np.stack([gen("heavy_f32", 50 + i, (k_out, N)) for i in range(count)])
    gates = packed.pack_batch(wg, np.stack([random_map((N, K), 33 + i) for i in range(count)]))
    ups = packed.pack_batch(wu, np.stack([random_map((N, K), 43 + i) for i in range(count)]))
    downs = packed.pack_batch(wd, np.stack([random_map((k_out, N), 53 + i) for i in range(count)]))
    return gates, ups, downs


def test_the_emulation_of_glu_grouped_skinny_is_glu_grouped():
    count, rows = 3, [0, 5, 5, 21]
    gates, ups, _downs = _experts(count)
    x = to_bf16_valued(gen("normal_f32", 29, (rows[-1], K)) * 4)
    bg, bu = gen("normal_f32", 31, (count, N)), gen("normal_f32", 32, (count, N))
    for act in packed.ACTS:
        for b_g, b_u in ((None, None), (bg, bu)):
            want = packed.glu_grouped(x, rows, gates, ups, act=act, bias_gate=b_g, bias_up=b_u)
            for split in (0, 2):
                got = packed.glu_grouped_skinny(x, rows, gates, ups, act=act, bias_gate=b_g, bias_up=b_u, split=split)
                assert got.shape == (21, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (act, split)
    hb16 = packed.glu_grouped_skinny(torch.from_numpy(x).to(torch.bfloat16), rows, gates, ups, out_dtype="bfloat16")
    assert torch.equal(hb16.view(torch.int16), packed.glu_grouped(x, rows, gates, ups, out_dtype="bfloat16").view(torch.int16))
    assert packed.glu_grouped_skinny(x[:0], [0] * (count + 1), gates, ups).shape == (0, N)
    with pytest.raises(hb.MtqError, match="as many experts"):
        packed.glu_grouped_skinny(x, rows, gates, ups[:2])
    with pytest.raises(hb.MtqError, match="group_rows"):
        packed.glu_grouped_skinny(x, [0, 5, 4, 21], gates, ups)
    with pytest.raises(hb.MtqError, match="act must be"):
        packed.glu_grouped_skinny(x, rows, gates, ups, act="gelu")
    # the names the older tests pin are as they were, and "skinny" is no name of glu_grouped
    assert packed.GLU_KERNELS == ("fused", "unfused", "auto") and packed.GLU_GROUPED_KERNELS == ("fused", "unfused")
    for kernel in ("skinny", "auto"):
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.glu_grouped(x, rows, gates, ups, kernel=kernel)


# ----------------------------------------------------------------------------- routing

def test_packed_mlp_routes_decode_through_glu_skinny_only_when_asked(monkeypatch):
    gate, up = _pair()
    down = packed.pack(gen("heavy_f32", 3, (64, N)), random_map((64, N), 4))
    calls = []

    def linear_recorder(name):
        def record(x, data, tables, n, bias=None, out_dtype=None, **kw):
            calls.append((name, tables, int(x.shape[0]), n, out_dtype))
            return torch.zeros((int(x.shape[0]), n), dtype=out_dtype)
        return record

    def fused_recorder(name):
        def record(x, gdata, gtables, udata, utables, n, act="silu", bias_gate=None, bias_up=None, out_dtype=None, **kw):
            calls.append((name, gtables, utables, int(x.shape[0]), n, act, out_dtype, kw))
            return torch.zeros((int(x.shape[0]), n), dtype=out_dtype)
        return record

    def combine(g, u, act="silu", out_dtype=None, **kw):
        calls.append(("combine", act, out_dtype))
        return torch.zeros(tuple(g.shape), dtype=out_dtype)

    for name in ("packed_linear", "packed_linear_skinny", "packed_linear_wide"):
        monkeypatch.setattr(hb, name, linear_recorder(name))
    monkeypatch.setattr(hb, "packed_glu_wide", fused_recorder("packed_glu_wide"))
    monkeypatch.setattr(hb, "packed_glu_skinny", fused_recorder("packed_glu_skinny"))
    monkeypatch.setattr(hb, "glu_combine", combine)
    monkeypatch.setattr(packed, "_device_data", lambda t: t.data)           # no upload: the recorders touch nothing
    gate._tables, up._tables, down._tables = "gate tables", "up tables", "down tables"

    def names(mlp, m):
        calls.clear()
        y = mlp(torch.zeros((m, K), dtype=torch.bfloat16))
        assert tuple(y.shape) == (m, 64)
        return [c[0] for c in calls]

    default = packed.PackedMLP(gate, up, down, backend="hip")
    assert default.decode_kernel == "pair" and packed.PackedMLP(gate, up, down, backend="hip", decode_kernel="pair").decode_kernel == "pair"
    fused = packed.PackedMLP(gate, up, down, backend="hip", decode_kernel="fused")
    top = packed.AUTO_SKINNY_MAX_M
    pair_route = ["packed_linear_skinny", "packed_linear_skinny", "combine", "packed_linear_skinny"]
    for m in (1, 7, top):
        assert names(default, m) == pair_route, m         # today's route: two skinny calls, the combine, the down projection
        assert calls[0][1:] == ("gate tables", m, N, torch.float32) and calls[1][1:] == ("up tables", m, N, torch.float32)
        assert names(fused, m) == ["packed_glu_skinny", "packed_linear_skinny"], m
        assert calls[0][:7] == ("packed_glu_skinny", "gate tables", "up tables", m, N, "silu", torch.bfloat16)
        assert calls[0][7].get("split", 0) == 0 and calls[1][1:] == ("down tables", m, 64, torch.bfloat16)
    for m in (top + 1, 40, 300):                          # above the decode range the option changes nothing
        assert names(fused, m) == names(default, m) and "packed_glu_skinny" not in names(fused, m), m
    assert names(packed.PackedMLP(gate, up, down, backend="hip", decode_kernel="fused", act="none"), 3) == ["packed_glu_skinny", "packed_linear_skinny"]
    assert calls[0][5] == "none"
    # glu(kernel="auto") itself goes where it went
    calls.clear()
    packed.glu(torch.zeros((5, K), dtype=torch.bfloat16), gate, up, backend="hip", kernel="auto")
    assert [c[0] for c in calls] == ["packed_linear_skinny", "packed_linear_skinny", "combine"]
    for bad in ("skinny", "auto", None, ""):
        with pytest.raises(hb.MtqError, match="decode_kernel must be one of"):
            packed.PackedMLP(gate, up, down, decode_kernel=bad)
    with pytest.raises(hb.MtqError, match="m <= 32"):     # the function itself refuses what the module never sends
        packed.glu_skinny(torch.zeros((33, K), dtype=torch.bfloat16), gate, up, backend="hip")
    # on emulation both settings give the same bits
    x = torch.from_numpy(to_bf16_valued(gen("normal_f32", 25, (7, K)) * 4)).to(torch.bfloat16)
    a = packed.PackedMLP(gate, up, down, backend="emulation")(x)
    b = packed.PackedMLP(gate, up, down, backend="emulation", decode_kernel="fused")(x)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_packed_experts_mlp_routes_decode_through_glu_grouped_skinny_only_when_asked(monkeypatch):
    count = 3
    gates, ups, downs = _experts(count)
    calls = []

    def record(name):
        def fn(x, group_rows, *args, **kw):
            calls.append((name, int(x.shape[0]), kw))
            return torch.zeros((int(x.shape[0]), 64 if args and args[0] is downs_b else N), dtype=torch.bfloat16)
        return fn

    gates_b, ups_b, downs_b = (packed.as_batch(b) for b in (gates, ups, downs))
    for name in ("glu_grouped", "glu_grouped_skinny", "linear_grouped", "linear_grouped_wide"):
        monkeypatch.setattr(packed, name, record(name))

    def names(mlp, T):
        calls.clear()
        mlp(torch.zeros((T, K), dtype=torch.bfloat16), [0, T, T, T])
        return [c[0] for c in calls]

    default = packed.PackedExpertsMLP(gates_b, ups_b, downs_b)
    assert default.decode_max_rows is None
    decode = packed.PackedExpertsMLP(gates_b, ups_b, downs_b, decode_max_rows=64)
    assert decode.decode_max_rows == 64
    for T in (1, 21, 64, 65, 300):
        assert names(default, T) == ["glu_grouped", "linear_grouped_wide"], T
        assert calls[0][2]["kernel"] == "fused"
    for T in (1, 21, 64):
        assert names(decode, T) == ["glu_grouped_skinny", "linear_grouped"], T
        assert calls[0][2]["out_dtype"] == "bfloat16" and calls[0][2].get("split", 0) == 0 and calls[1][2]["kernel"] == "walk"
        assert calls[1][2].get("split", 0) == 0
    for T in (65, 70, 300):
        assert names(decode, T) == ["glu_grouped", "linear_grouped_wide"], T
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(hb.MtqError, match="decode_max_rows"):
            packed.PackedExpertsMLP(gates_b, ups_b, downs_b, decode_max_rows=bad)


def test_packed_experts_mlp_on_emulation_is_the_written_out_composition():
    count, rows = 3, [0, 5, 5, 21]
    gates, ups, downs = _experts(count)
    xt = torch.from_numpy(to_bf16_valued(gen("normal_f32", 29, (rows[-1], K)) * 4)).to(torch.bfloat16)
    mlp = packed.PackedExpertsMLP(gates, ups, downs, decode_max_rows=21)
    h = packed.glu_grouped_skinny(xt, rows, gates, ups, out_dtype="bfloat16")
    want = packed.linear_grouped(h, rows, downs, out_dtype="bfloat16", kernel="walk")
    y = mlp(xt, rows)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (21, 64) and torch.equal(y.view(torch.int16), want.view(torch.int16))
    assert mlp._decode_workspace is None and tuple(mlp(xt[:0], [0] * (count + 1)).shape) == (0, 64)
