"""CPU-only: the gated product on packed weights (packed.glu, packed.glu_grouped, PackedMLP, PackedExpertsMLP) as far as it goes
without a device.  The three C entries and the size function are declared, optional and exported; each refuses bad arguments with
MTQ_ERR_INVALID before a device is looked for, and an unknown activation code with MTQ_ERR_UNSUPPORTED; the emulation is a float64
expression written out here; gate / up mismatches raise; kernel="auto" reaches the expected bindings (replaced by recorders: nothing
here needs a GPU); and max |silu'| < 1.1, the constant of the GPU tests' accuracy bound."""
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

HEADER = Path(__file__).resolve().parents[1] / "include" / "mtq.h"
GLU = ("mtq_glu_combine", "mtq_packed_glu_wide", "mtq_packed_glu_wide_grouped", "mtq_packed_glu_wide_grouped_workspace_bytes")
INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -3


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def test_the_entries_are_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    for name in GLU:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name) is not None
    assert re.search(r"enum \{ MTQ_ACT_SILU = 0, MTQ_ACT_NONE = 1 \}", text) and hb.ACT_CODE == {"silu": 0, "none": 1}
    assert set(hb.PACKED_GLU) == set(GLU) and hb.has_packed_glu() is True
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    assert hb.SIGNATURES[GLU[3]][:2] == hb.SIGNATURES["mtq_packed_linear_wide_grouped_workspace_bytes"][:2]
    for args in ((70, 5, 72, 300), (1, 1, 40, 100), (512, 300, 2048, 7168)):      # the wide grouped entry's plan workspace
        assert hb.packed_glu_wide_grouped_workspace_bytes(*args) == hb.packed_linear_wide_grouped_workspace_bytes(*args)
    assert hb._entry(GLU[3])(0, 5, 72, 300) == 2 ** 64 - 1


def test_a_build_without_the_entries_still_loads(monkeypatch):
    stub = _StubLibrary(143, missing=GLU)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_linear_wide_grouped.argtypes is not None             # every other symbol is bound
    assert not hb.has_packed_glu()
    for name in GLU:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    pt = packed.pack(gen("heavy_f32", 1, (40, 100)), random_map((40, 100), 2))
    x = torch.zeros((40, 100), dtype=torch.bfloat16)
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_wide.*lacks"):        # no other kernel in its place
        packed.glu(x, pt, pt, backend="hip", kernel="unfused")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_wide.*lacks"):
        packed.PackedMLP(pt, pt, packed.pack(gen("heavy_f32", 3, (64, 40)), random_map((64, 40), 4)), backend="hip")


def test_glu_combine_checks_its_arguments_before_a_device():
    fn = hb._entry("mtq_glu_combine")
    _buf, p = _aligned()

    def call(g=p, ldg=70, u=p, ldu=70, rows=8, cols=70, act=0, y=p, dtype=hb.DTYPE_F32, ldy=70):
        return fn(g, ldg, u, ldu, rows, cols, act, y, dtype, ldy, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("g", "u", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=7)
    refused("must be positive", rows=0)
    refused("must be positive", rows=-2)
    refused("must be positive", cols=0, ldg=0, ldu=0, ldy=0)
    refused("ldg < cols", ldg=69)
    refused("ldu < cols", ldu=69)
    refused("ldy < cols", ldy=69)
    refused("too large", rows=(1 << 40) + 1)
    refused("too large", rows=1 << 40, cols=1 << 20, ldg=1 << 20, ldu=1 << 20, ldy=1 << 20)
    for act in (2, -1, 7):
        assert call(act=act) == UNSUPPORTED and "act must be" in _last()
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert call() == NO_DEVICE and call(act=1, dtype=hb.DTYPE_BF16) == NO_DEVICE


def test_glu_wide_checks_both_streams_before_a_device():
    fn = hb._entry("mtq_packed_glu_wide")
    _buf, p = _aligned()
    m, n, k = 300, 64, 64                                 # 2 x 2 tiles: at least 4 * 320 bytes a stream

    def call(x=p, m=m, k=k, ldx=k, gp=p, gbytes=1 << 20, gmap=p, goff=p, up=p, ubytes=1 << 20, umap=p, uoff=p, n=n, bg=None, bu=None, act=0, y=p,
             dtype=hb.DTYPE_F32, ldy=n):
        return fn(x, m, k, ldx, gp, gbytes, gmap, goff, up, ubytes, umap, uoff, n, bg, bu, act, y, dtype, ldy, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "gp", "gmap", "goff", "up", "umap", "uoff", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=5)
    refused("out_dtype", dtype=-1)
    refused("m must be positive", m=0)
    refused("m must be positive", m=-3)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", n=-1)
    refused("rows and cols must be positive", k=0)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("matrix too large", m=(1 << 40) + 1)
    refused("matrix too large", n=(1 << 30) + 1, ldy=1 << 31)
    refused("matrix too large", k=(1 << 30) + 1, ldx=1 << 31)
    refused("packed must be 16-byte aligned", gp=p + 8)
    refused("packed must be 16-byte aligned", up=p + 8)
    refused("smaller than the stream", gbytes=4 * 320 - 1)
    refused("smaller than the stream", ubytes=4 * 320 - 1)
    refused("smaller than the stream", ubytes=0)
    refused("too many workgroups", m=1 << 40, n=1 << 20, ldy=1 << 20, gbytes=1 << 40, ubytes=1 << 40)
    for act in (2, -1):
        assert call(act=act) == UNSUPPORTED and "act must be" in _last()
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(m=1, act=1, bg=p, bu=p) == NO_DEVICE


def test_glu_wide_grouped_checks_both_arenas_before_a_device():
    fn = hb._entry("mtq_packed_glu_wide_grouped")
    _buf, p = _aligned()
    T, count, n, k = 8, 2, 40, 70                         # 2 x 3 tiles each: at least 12 * 320 bytes an arena
    need = hb.packed_glu_wide_grouped_workspace_bytes(T, count, n, k)
    assert need == 16

    def call(x=p, T=T, k=k, ldx=k, rows=p, gp=p, gbytes=12 * 320, gmaps=p, goffs=p, gbases=p, up=p, ubytes=12 * 320, umaps=p, uoffs=p, ubases=p,
             count=count, n=n, bg=None, bu=None, ldb=n, act=0, y=p, dtype=hb.DTYPE_F32, ldy=n, ws=p, ws_bytes=1 << 15):
        return fn(x, T, k, ldx, rows, gp, gbytes, gmaps, goffs, gbases, up, ubytes, umaps, uoffs, ubases, count, n, bg, bu, ldb, act, y, dtype, ldy,
                  ws, ws_bytes, None)

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
    refused("workspace is null", ws=None, ws_bytes=0)
    refused("workspace is null", ws=None)
    refused("workspace must be 16-byte aligned", ws=p + 4)
    refused("smaller than the", ws_bytes=need - 1)
    for act in (2, -1):
        assert call(act=act) == UNSUPPORTED and "act must be" in _last()
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(ldb=n - 1) == NO_DEVICE         # without a bias ldb means nothing


# ----------------------------------------------------------------------------- the emulation

N, K = 40, 100


def _pair(n=N, k=K):
    wg, wu = gen("heavy_f32", 21, (n, k)), gen("heavy_f32", 22, (n, k))
    return packed.pack(wg, random_map((n, k), 23)), packed.pack(wu, random_map((n, k), 24))


def _weights64(pt):
    return packed.unpack(pt).astype(np.float64)


def test_the_emulation_is_the_float64_expression():
    gate, up = _pair()
    x = to_bf16_valued(gen("normal_f32", 25, (37, K)) * 4)
    bg, bu = gen("normal_f32", 26, (N,)), gen("normal_f32", 27, (N,))
    x64 = x.astype(np.float64)
    for b_g, b_u in ((None, None), (bg, None), (None, bu), (bg, bu)):
        g64 = x64 @ _weights64(gate).T + (0.0 if b_g is None else b_g.astype(np.float64)[None, :])
        u64 = x64 @ _weights64(up).T + (0.0 if b_u is None else b_u.astype(np.float64)[None, :])
        for act, h64 in (("silu", g64 / (1.0 + np.exp(-g64)) * u64), ("none", g64 * u64)):
            want = h64.astype(np.float32)
            for kernel in packed.GLU_KERNELS:
                got = packed.glu(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, kernel=kernel)
                assert got.shape == (37, N) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (act, kernel)
            assert np.array_equal(packed.glu_emulation_f64(x, gate, up, act, b_g, b_u), h64)
            yb = packed.glu(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, out_dtype="bfloat16", backend="emulation")
            assert yb.dtype == torch.bfloat16 and torch.equal(yb.view(torch.int16), torch.from_numpy(want).to(torch.bfloat16).view(torch.int16))
    assert not np.array_equal(packed.glu(x, gate, up), packed.glu(x, up, gate))          # the two streams are not interchangeable
    assert packed.glu(x[:0], gate, up).shape == (0, N)
    assert packed.glu(torch.from_numpy(x).to(torch.bfloat16), gate, up).dtype == np.float32


def test_the_grouped_emulation_and_the_modules_are_the_written_out_compositions():
    count, rows = 3, [0, 5, 5, 21]
    wg = np.stack([gen("heavy_f32", 30 + i, (N, K)) for i in range(count)])
    wu = np.stack([gen("heavy_f32", 40 + i, (N, K)) for i in range(count)])
    wd = np.stack([gen("heavy_f32", 50 + i, (64, N)) for i in range(count)])
    gates = packed.pack_batch(wg, np.stack([random_map((N, K), 33 + i) for i in range(count)]))
    ups = packed.pack_batch(wu, np.stack([random_map((N, K), 43 + i) for i in range(count)]))
    downs = packed.pack_batch(wd, np.stack([random_map((64, N), 53 + i) for i in range(count)]))
    x = to_bf16_valued(gen("normal_f32", 29, (rows[-1], K)) * 4)
    bg, bu = gen("normal_f32", 31, (count, N)), gen("normal_f32", 32, (count, N))
    for act in packed.ACTS:
        got = packed.glu_grouped(x, rows, gates, ups, act=act, bias_gate=bg, bias_up=bu)
        for kernel in packed.GLU_GROUPED_KERNELS:
            assert np.array_equal(packed.glu_grouped(x, rows, gates, ups, act=act, bias_gate=bg, bias_up=bu, kernel=kernel).view(np.uint32), got.view(np.uint32))
        for e in range(count):
            want = packed.glu(x[rows[e]:rows[e + 1]], gates[e], ups[e], act=act, bias_gate=bg[e], bias_up=bu[e])
            assert np.array_equal(got[rows[e]:rows[e + 1]].view(np.uint32), want.view(np.uint32)), (act, e)
    xt = torch.from_numpy(x).to(torch.bfloat16)
    mlp = packed.PackedExpertsMLP(gates, ups, downs)
    assert mlp.backend == "emulation" and (mlp.count, mlp.in_features, mlp.hidden_features, mlp.out_features) == (count, K, N, 64)
    h = packed.glu_grouped(xt, rows, gates, ups, out_dtype="bfloat16")
    want = packed.linear_grouped_wide(h, rows, downs, out_dtype="bfloat16")
    y = mlp(xt, rows)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (rows[-1], 64) and torch.equal(y.view(torch.int16), want.view(torch.int16))
    assert tuple(mlp(xt[:0], [0] * (count + 1)).shape) == (0, 64)
    dense = packed.PackedMLP(gates[0], ups[0], downs[0], act="none", out_dtype="float32")
    h = packed.glu(xt, gates[0], ups[0], act="none", out_dtype="bfloat16")
    want = packed.linear(h, downs[0])
    y = dense(xt.reshape(3, 7, K))
    assert y.dtype == torch.float32 and tuple(y.shape) == (3, 7, 64) and np.array_equal(y.reshape(21, 64).numpy().view(np.uint32), want.view(np.uint32))
    assert tuple(dense(xt[:0]).shape) == (0, 64)
    with pytest.raises(hb.MtqError, match="down"):
        packed.PackedMLP(gates[0], ups[0], gates[0])
    with pytest.raises(hb.MtqError, match="down batch"):
        packed.PackedExpertsMLP(gates, ups, gates)
    with pytest.raises(hb.MtqError, match="as many experts"):
        packed.glu_grouped(x, rows, gates, ups[:2])
    with pytest.raises(hb.MtqError, match="group_rows"):
        packed.glu_grouped(x, [0, 5, 4, 21], gates, ups)
    with pytest.raises(hb.MtqError, match="kernel"):
        packed.glu_grouped(x, rows, gates, ups, kernel="auto")


def test_mismatched_gate_and_up_are_refused():
    gate, up = _pair()
    x = to_bf16_valued(gen("normal_f32", 25, (4, K)))
    other = packed.pack(gen("heavy_f32", 1, (N, K + 32)), random_map((N, K + 32), 2))
    taller = packed.pack(gen("heavy_f32", 1, (N + 1, K)), random_map((N + 1, K), 2))     # the same tile grid, another n
    cube = packed.pack(gen("normal_f32", 1, (2, 20, K)), random_map((N, K), 2))
    for backend in (None, "emulation", "hip"):
        for g, u, word in ((gate, other, "one shape"), (other, up, "one shape"), (gate, taller, "one shape"), (cube, up, "2-D"), (gate, cube, "2-D")):
            with pytest.raises(hb.MtqError, match=word):
                packed.glu(x, g, u, backend=backend)
        with pytest.raises(hb.MtqError, match="act must be"):
            packed.glu(x, gate, up, act="gelu", backend=backend)
        with pytest.raises(hb.MtqError, match="kernel must be"):
            packed.glu(x, gate, up, kernel="block", backend=backend)
        with pytest.raises(hb.MtqError, match="out_dtype"):
            packed.glu(x, gate, up, out_dtype="float16", backend=backend)
    with pytest.raises(hb.MtqError, match="x must be"):
        packed.glu(x[:, :64], gate, up)
    with pytest.raises(hb.MtqError, match="bias_up must be"):
        packed.glu(x, gate, up, bias_up=np.zeros(N + 1, dtype=np.float32))
    turned = packed.pack(gen("heavy_f32", 22, (N, K)), random_map((N, K), 24))
    turned.layout = "transpose"
    for g, u in ((gate, turned), (turned, up)):
        with pytest.raises(hb.MtqError, match="row layout"):
            packed.glu(x, g, u)


def test_auto_reaches_the_expected_bindings(monkeypatch):
    gate, up = _pair()
    calls = []

    def linear_recorder(name):
        def record(x, data, tables, n, bias=None, out_dtype=None, **kw):
            calls.append((name, tables, int(x.shape[0]), n, out_dtype))
            return (name, tables)
        return record

    def fused(x, gdata, gtables, udata, utables, n, act="silu", bias_gate=None, bias_up=None, out_dtype=None, **kw):
        calls.append(("fused", gtables, utables, int(x.shape[0]), n, act, out_dtype))
        return "fused"

    def combine(g, u, act="silu", out_dtype=None, **kw):
        calls.append(("combine", g, u, act, out_dtype))
        return "combined"

    monkeypatch.setattr(hb, "packed_linear", linear_recorder("block"))
    monkeypatch.setattr(hb, "packed_linear_skinny", linear_recorder("skinny"))
    monkeypatch.setattr(hb, "packed_linear_wide", linear_recorder("wide"))
    monkeypatch.setattr(hb, "packed_glu_wide", fused)
    monkeypatch.setattr(hb, "glu_combine", combine)
    monkeypatch.setattr(packed, "_device_data", lambda t: t.data)           # no upload: the recorders touch nothing
    gate._tables, up._tables = "gate tables", "up tables"

    def routed(m, kernel="auto", act="silu"):
        calls.clear()
        x = torch.zeros((m, K), dtype=torch.bfloat16)
        got = packed.glu(x, gate, up, act=act, out_dtype="bfloat16", backend="hip", kernel=kernel)
        if got == "fused":
            assert calls == [("fused", "gate tables", "up tables", m, N, act, torch.bfloat16)]
            return "fused"
        family = calls[0][0]
        # two projections into float32, the gate's first, then the combine of exactly those two into the asked type
        assert got == "combined" and calls == [(family, "gate tables", m, N, torch.float32), (family, "up tables", m, N, torch.float32),
                                               ("combine", (family, "gate tables"), (family, "up tables"), act, torch.bfloat16)]
        return family

    skinny_max, gate_m = packed.AUTO_SKINNY_MAX_M, packed.AUTO_GLU_FUSED_MIN_M
    assert gate_m is None or (isinstance(gate_m, int) and gate_m > skinny_max)
    assert routed(1) == "skinny" and routed(skinny_max) == "skinny" and routed(1, act="none") == "skinny"
    if gate_m is None:
        assert routed(skinny_max + 1) == "block" and routed(4096) == "block" and routed(1 << 16) == "block"
    else:
        assert routed(gate_m - 1) == ("block" if gate_m - 1 > skinny_max else "skinny")
        assert routed(gate_m) == "fused" and routed(gate_m + 1) == "fused" and routed(8 * gate_m, act="none") == "fused"
        assert routed(skinny_max + 1) == ("block" if gate_m > skinny_max + 1 else "fused")
    for m in (1, 33, 4096):                               # the explicit names go where they say at every m
        assert routed(m, kernel="fused") == "fused" and routed(m, kernel="unfused") == "block"


def test_the_slope_of_silu_is_below_the_bounds_constant():
    g = np.linspace(-30.0, 30.0, 6_000_001)
    s = 1.0 / (1.0 + np.exp(-g))
    slope = s * (1.0 + g * (1.0 - s))
    assert packed.GLU_SILU_SLOPE_MAX == 1.1                # the constant of the GPU tests' bound, in one place
    assert g.dtype == np.float64 and np.abs(slope).max() < packed.GLU_SILU_SLOPE_MAX
    assert np.abs(slope).max() > 1.099                    # and the constant is not slack: the maximum is 1.09984 near g = 2.4
    # outside the grid |silu'| only falls towards 1 and 0: silu' - 1 = s (g (1 - s)) - (1 - s) is positive and decreasing for g > 30
    assert abs(slope[-1] - 1.0) < 1e-11 and abs(slope[0]) < 1e-11
