"""CPU-only: the gated product over packed (k, n) weights (packed.glu_matmul, glu_matmul_skinny, glu_matmul_grouped,
glu_matmul_grouped_skinny, PackedMatmulMLP, PackedExpertsMatmulMLP, PackedMoE(stored="transpose")) as far as it goes without a device.
The seven C symbols are declared, optional and exported, with the parameter lists of the mtq_packed_glu_* entries of the same name; the
size functions equal the linear family's on a grid of arguments; every refusal of the C entries comes back before a device is looked for
(the pointers handed in are host addresses that no check may dereference); the emulation of the four functions and the three modules is
the float64 composition written out here; a library without the symbols raises MtqError and nothing stands in."""
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
WIDE = ("mtq_packed_glu_matmul_wide", "mtq_packed_glu_matmul_wide_grouped", "mtq_packed_glu_matmul_wide_grouped_workspace_bytes")
SKINNY = ("mtq_packed_glu_matmul_skinny_workspace_bytes", "mtq_packed_glu_matmul_skinny", "mtq_packed_glu_matmul_skinny_grouped_workspace_bytes",
          "mtq_packed_glu_matmul_skinny_grouped")
NEW = WIDE + SKINNY
INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -3
BAD_SIZE = 2 ** 64 - 1
N, K, K_OUT = 40, 100, 64                                # hidden, contraction, the down projection's width


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def test_the_entries_are_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name) is not None
        # the parameter list of the linear-family entry of the same name, one for one
        assert hb.SIGNATURES[name][:2] == hb.SIGNATURES[name.replace("_glu_matmul_", "_glu_")][:2], name
    assert set(hb.PACKED_GLU_MATMUL) == set(WIDE) and set(hb.PACKED_GLU_MATMUL_SKINNY) == set(SKINNY)
    assert hb.has_packed_glu_matmul() is True and hb.has_packed_glu_matmul_skinny() is True
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    assert packed.AUTO_GLU_MATMUL_SKINNY_MAX_M == 32 and packed.MOE_STORED == ("rows", "transpose")


def _kn_pair(n=N, k=K):
    wg, wu = gen("heavy_f32", 21, (n, k)), gen("heavy_f32", 22, (n, k))
    return packed.pack_transposed(wg, random_map((k, n), 23)), packed.pack_transposed(wu, random_map((k, n), 24))


def _kn_down():
    return packed.pack_transposed(gen("heavy_f32", 3, (K_OUT, N)), random_map((N, K_OUT), 4))


def _kn_experts(count=3):
    wg = np.stack([gen("heavy_f32", 30 + i, (N, K)) for i in range(count)])
    wu = np.stack([gen("heavy_f32", 40 + i, (N, K)) for i in range(count)])
    wd = np.stack([gen("heavy_f32", 50 + i, (K_OUT, N)) for i in range(count)])
    gates = packed.pack_batch_transposed(wg, np.stack([random_map((K, N), 33 + i) for i in range(count)]))
    ups = packed.pack_batch_transposed(wu, np.stack([random_map((K, N), 43 + i) for i in range(count)]))
    downs = packed.pack_batch_transposed(wd, np.stack([random_map((N, K_OUT), 53 + i) for i in range(count)]))
    return gates, ups, downs


def test_a_build_without_the_entries_still_loads_and_nothing_stands_in(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_skinny_grouped.argtypes is not None               # every other symbol is bound
    assert hb.has_packed_glu() and hb.has_packed_glu_skinny() and not hb.has_packed_glu_matmul() and not hb.has_packed_glu_matmul_skinny()
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    gate, up = _kn_pair()
    down = _kn_down()
    gates, ups, downs = _kn_experts(1)
    x = torch.zeros((4, K), dtype=torch.bfloat16)
    for kernel in packed.GLU_KERNELS:
        with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_wide.*lacks.*rebuild it from this tree"):
            packed.glu_matmul(x, gate, up, backend="hip", kernel=kernel)
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_skinny.*lacks.*rebuild it from this tree"):
        packed.glu_matmul_skinny(x, gate, up, backend="hip")
    for kernel in packed.GLU_GROUPED_KERNELS:
        with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_wide_grouped.*lacks"):
            packed.glu_matmul_grouped(x, [0, 4], gates, ups, backend="hip", kernel=kernel)
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_skinny_grouped.*lacks"):
        packed.glu_matmul_grouped_skinny(x, [0, 4], gates, ups, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_wide.*lacks"):
        packed.PackedMatmulMLP(gate, up, down, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_wide.*lacks"):
        packed.PackedExpertsMatmulMLP(gates, ups, downs, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_wide.*lacks"):
        packed.PackedMoE(gates, ups, downs, backend="hip", stored="transpose")
    stub = _StubLibrary(143, missing=SKINNY)             # the wide entries alone: the decode options are refused where they are asked for
    assert _load(monkeypatch, stub) is stub and hb.has_packed_glu_matmul() and not hb.has_packed_glu_matmul_skinny()
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_skinny.*lacks"):
        packed.PackedMatmulMLP(gate, up, down, backend="hip", decode_kernel="fused")
    with pytest.raises(hb.MtqError, match="mtq_packed_glu_matmul_skinny.*lacks"):
        packed.PackedExpertsMatmulMLP(gates, ups, downs, backend="hip", decode_max_rows=8)


def test_the_size_functions_equal_the_linear_family_on_a_grid():
    for m in (1, 5, 32):
        for n in (1, 33, 40, 96, 4096):
            for k in (1, 32, 100, 2080, 14336):
                for split in (0, 1, 2, 3, 1000):
                    got = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, split)
                    assert got == hb.packed_glu_skinny_workspace_bytes(m, n, k, split) > 0, (m, n, k, split)
    for T in (1, 21, 70, 4096):
        for count in (1, 3, 64, 256):
            for n, k in ((40, 100), (96, 288), (2048, 7168), (32, 32)):
                assert (hb.packed_glu_matmul_wide_grouped_workspace_bytes(T, count, n, k) == hb.packed_glu_wide_grouped_workspace_bytes(T, count, n, k)
                        == (4 * (count + 1) + 15) // 16 * 16)
                for split in (0, 1, 2, 1000):
                    got = hb.packed_glu_matmul_skinny_grouped_workspace_bytes(T, count, n, k, split)
                    assert got == hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, split) > 0, (T, count, n, k, split)
    dense, grouped, wide = hb._entry(SKINNY[0]), hb._entry(SKINNY[2]), hb._entry(WIDE[2])
    for bad in ((0, 40, 100, 0), (33, 40, 100, 0), (-1, 40, 100, 0), (5, 0, 100, 0), (5, 40, 0, 0), (5, 40, 100, -1), (5, (1 << 30) + 1, 100, 0)):
        assert dense(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.packed_glu_matmul_skinny_workspace_bytes(*bad)
    for bad in ((0, 3, 40, 100, 0), (2 ** 31, 3, 40, 100, 0), (21, 0, 40, 100, 0), (21, 2 ** 31, 40, 100, 0), (21, 3, 0, 100, 0), (21, 3, 40, 0, 0),
                (21, 3, 40, 100, -1), (2 ** 31 - 1, 1, 1 << 30, 32, 1)):
        assert grouped(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.packed_glu_matmul_skinny_grouped_workspace_bytes(*bad)
    for bad in ((0, 3, 40, 100), (21, 0, 40, 100), (21, 3, 0, 100), (21, 3, 40, 0)):
        assert wide(*bad) == BAD_SIZE, bad
        with pytest.raises(hb.MtqError):
            hb.packed_glu_matmul_wide_grouped_workspace_bytes(*bad)


def _single_calls():
    """(name, call(**kw)) of the two single-tensor entries over one keyword set; the wide one drops split and the workspace."""
    _buf, p = _aligned()
    m, n, k = 8, 64, 64                                   # 2 x 2 tiles: at least 4 * 320 bytes a stream

    def make(name):
        fn = hb._entry(name)

        def call(x=p, m=m, k=k, ldx=k, gp=p, gbytes=1 << 20, gmap=p, goff=p, up=p, ubytes=1 << 20, umap=p, uoff=p, n=n, bg=None, bu=None, act=0, y=p,
                 dtype=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
            head = (x, m, k, ldx, gp, gbytes, gmap, goff, up, ubytes, umap, uoff, n, bg, bu, act, y, dtype, ldy)
            return fn(*head, None) if name == WIDE[0] else fn(*head, split, ws, ws_bytes, None)
        return call
    return p, m, n, k, {name: make(name) for name in (WIDE[0], SKINNY[1])}


def test_the_single_tensor_entries_refuse_before_a_device():
    p, m, n, k, calls = _single_calls()
    for name, call in calls.items():
        def refused(match, **kw):
            assert call(**kw) == INVALID, (name, kw)
            assert match in _last(), (name, _last())

        for arg in ("x", "gp", "gmap", "goff", "up", "umap", "uoff", "y"):
            refused("null argument", **{arg: None})
        refused("out_dtype", dtype=5)
        refused("m must be positive", m=0)
        refused("m must be positive", m=-3)
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
        for act in (2, -1, 7):
            assert call(act=act) == UNSUPPORTED and "act must be" in _last(), name
        if name == SKINNY[1]:
            refused("m > 32", m=33)
            refused("split must not be negative", split=-1)
            for split in (0, 1, 2, 1000):                 # the workspace at every split, split 1 included
                size = hb.packed_glu_matmul_skinny_workspace_bytes(m, n, k, split)
                refused("workspace is null", split=split, ws=None, ws_bytes=0)
                refused("workspace must be 16-byte aligned", split=split, ws=p + 4)
                refused("smaller than the", split=split, ws_bytes=size - 1)
        if not torch.cuda.is_available():                 # everything in order: only the device is missing
            assert call() == NO_DEVICE and call(m=1, act=1, bg=p, bu=p, dtype=hb.DTYPE_BF16) == NO_DEVICE, name


def test_the_grouped_entries_refuse_before_a_device():
    _buf, p = _aligned()
    T, count, n, k = 8, 2, 40, 70                         # 3 x 2 tiles each: at least 12 * 320 bytes an arena
    for name in (WIDE[1], SKINNY[3]):
        fn = hb._entry(name)

        def call(x=p, T=T, k=k, ldx=k, rows=p, gp=p, gbytes=12 * 320, gmaps=p, goffs=p, gbases=p, up=p, ubytes=12 * 320, umaps=p, uoffs=p,
                 ubases=p, count=count, n=n, bg=None, bu=None, ldb=n, act=0, y=p, dtype=hb.DTYPE_F32, ldy=n, split=0, ws=p, ws_bytes=1 << 15):
            head = (x, T, k, ldx, rows, gp, gbytes, gmaps, goffs, gbases, up, ubytes, umaps, uoffs, ubases, count, n, bg, bu, ldb, act, y, dtype, ldy)
            return fn(*head, ws, ws_bytes, None) if name == WIDE[1] else fn(*head, split, ws, ws_bytes, None)

        def refused(match, **kw):
            assert call(**kw) == INVALID, (name, kw)
            assert match in _last(), (name, _last())

        for arg in ("x", "rows", "gp", "gmaps", "goffs", "gbases", "up", "umaps", "uoffs", "ubases", "y"):
            refused("null argument", **{arg: None})
        refused("out_dtype", dtype=7)
        refused("total_rows must be positive", T=0)
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
        refused("workspace must be 16-byte aligned", ws=p + 4)
        if name == SKINNY[3]:
            refused("split must not be negative", split=-2)
            for split in (0, 1, 2):
                refused("smaller than the", split=split, ws_bytes=hb.packed_glu_matmul_skinny_grouped_workspace_bytes(T, count, n, k, split) - 1)
        else:
            refused("smaller than the", ws_bytes=hb.packed_glu_matmul_wide_grouped_workspace_bytes(T, count, n, k) - 1)
        for act in (2, -1):
            assert call(act=act) == UNSUPPORTED and "act must be" in _last(), name
        if not torch.cuda.is_available():
            assert call() == NO_DEVICE and call(ldb=n - 1) == NO_DEVICE, name    # without a bias ldb means nothing


# ----------------------------------------------------------------------------- the emulation: the float64 composition, written out

def _silu(g):
    with np.errstate(over="ignore", invalid="ignore"):
        return g / (1.0 + np.exp(-g))


def _f64(x, pt, bias):
    """X·unpack(P̂) + b in float64, on unpack's values."""
    w = packed.unpack(pt).astype(np.float64)              # (k, n)
    y = x.astype(np.float64) @ w
    return y if bias is None else y + np.asarray(bias, dtype=np.float64)[None, :]


def _glu64(x, gate, up, act, bg, bu):
    g, u = _f64(x, gate, bg), _f64(x, up, bu)
    return (g if act == "none" else _silu(g)) * u


def _round(h64, out_dtype="float32"):
    y = h64.astype(np.float32)
    return y if out_dtype == "float32" else torch.from_numpy(y).to(torch.bfloat16)


def test_the_emulation_of_glu_matmul_and_glu_matmul_skinny_is_the_float64_definition():
    gate, up = _kn_pair()
    assert gate.shape == (K, N)
    x = to_bf16_valued(gen("normal_f32", 25, (37, K)) * 4)
    bg, bu = gen("normal_f32", 26, (N,)), gen("normal_f32", 27, (N,))
    for b_g, b_u in ((None, None), (bg, None), (None, bu), (bg, bu)):
        for act in packed.ACTS:
            want64 = _glu64(x, gate, up, act, b_g, b_u)
            assert np.array_equal(packed.glu_matmul_emulation_f64(x, gate, up, act, b_g, b_u), want64)
            want = _round(want64)
            for kernel in packed.GLU_KERNELS:
                got = packed.glu_matmul(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, kernel=kernel)
                assert got.dtype == np.float32 and got.shape == (37, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            for split in (0, 1, 3):
                got = packed.glu_matmul_skinny(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, split=split)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            gb = packed.glu_matmul(x, gate, up, act=act, bias_gate=b_g, bias_up=b_u, out_dtype="bfloat16", backend="emulation")
            assert gb.dtype == torch.bfloat16 and torch.equal(gb.view(torch.int16), _round(want64, "bfloat16").view(torch.int16))
    # the linear family on the transposed weight computes the same float64 value
    rows = [packed.pack(np.ascontiguousarray(packed.unpack(pt).T), np.zeros(((N + 31) // 32, (K + 31) // 32), dtype=np.int8)) for pt in (gate, up)]
    assert np.array_equal(packed.glu(x, rows[0], rows[1], bias_gate=bg).view(np.uint32), packed.glu_matmul(x, gate, up, bias_gate=bg).view(np.uint32))
    assert packed.glu_matmul(x[:0], gate, up).shape == (0, N) and packed.glu_matmul_skinny(x[:0], gate, up).shape == (0, N)
    other = packed.pack_transposed(gen("heavy_f32", 1, (N, K + 32)), random_map((K + 32, N), 2))
    for fn in (packed.glu_matmul, packed.glu_matmul_skinny):
        for backend in (None, "emulation", "hip"):
            with pytest.raises(hb.MtqError, match="one shape"):
                fn(x, gate, other, backend=backend)
            with pytest.raises(hb.MtqError, match="act must be"):
                fn(x, gate, up, act="gelu", backend=backend)
            with pytest.raises(hb.MtqError, match="out_dtype"):
                fn(x, gate, up, out_dtype="float16", backend=backend)
        with pytest.raises(hb.MtqError, match="backend must be"):
            fn(x, gate, up, backend="cuda")
        with pytest.raises(hb.MtqError, match=rf"x must be \(m, {K}\)"):
            fn(x[:, :K - 1], gate, up)
    for kernel in ("skinny", "block", None):
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.glu_matmul(x, gate, up, kernel=kernel)


def _grouped64(x, rows, gates, ups, act, bg, bu):
    h = np.zeros((x.shape[0], N), dtype=np.float64)
    for e in range(len(gates)):
        r0, r1 = rows[e], rows[e + 1]
        if r1 > r0:
            h[r0:r1] = _glu64(x[r0:r1], gates[e], ups[e], act, None if bg is None else bg[e], None if bu is None else bu[e])
    return h


def test_the_emulation_of_the_grouped_functions_is_the_float64_definition_per_expert():
    count, rows = 3, [0, 5, 5, 21]
    gates, ups, _downs = _kn_experts(count)
    x = to_bf16_valued(gen("normal_f32", 29, (rows[-1], K)) * 4)
    bg, bu = gen("normal_f32", 31, (count, N)), gen("normal_f32", 32, (count, N))
    for act in packed.ACTS:
        for b_g, b_u in ((None, None), (bg, bu), (bg, None)):
            want = _round(_grouped64(x, rows, gates, ups, act, b_g, b_u))
            for kernel in packed.GLU_GROUPED_KERNELS:
                got = packed.glu_matmul_grouped(x, rows, gates, ups, act=act, bias_gate=b_g, bias_up=b_u, kernel=kernel)
                assert got.shape == (21, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (act, kernel)
            for split in (0, 2):
                got = packed.glu_matmul_grouped_skinny(x, rows, gates, ups, act=act, bias_gate=b_g, bias_up=b_u, split=split)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (act, split)
    h16 = packed.glu_matmul_grouped_skinny(torch.from_numpy(x).to(torch.bfloat16), rows, gates, ups, out_dtype="bfloat16")
    assert torch.equal(h16.view(torch.int16), _round(_grouped64(x, rows, gates, ups, "silu", None, None), "bfloat16").view(torch.int16))
    assert packed.glu_matmul_grouped(x[:0], [0] * (count + 1), gates, ups).shape == (0, N)
    assert packed.glu_matmul_grouped_skinny(x[:0], [0] * (count + 1), gates, ups).shape == (0, N)
    for fn in (packed.glu_matmul_grouped, packed.glu_matmul_grouped_skinny):
        with pytest.raises(hb.MtqError, match="as many experts"):
            fn(x, rows, gates, ups[:2])
        with pytest.raises(hb.MtqError, match="group_rows"):
            fn(x, [0, 5, 4, 21], gates, ups)
        with pytest.raises(hb.MtqError, match="act must be"):
            fn(x, rows, gates, ups, act="gelu")
        with pytest.raises(hb.MtqError, match=rf"x must be \(T, {K}\)"):
            fn(x[:, :N], rows, gates, ups)
    for kernel in ("skinny", "auto"):
        with pytest.raises(hb.MtqError, match="kernel must be one of"):
            packed.glu_matmul_grouped(x, rows, gates, ups, kernel=kernel)


def test_the_modules_on_emulation_are_their_written_out_compositions():
    gate, up = _kn_pair()
    down = _kn_down()
    xt = torch.from_numpy(to_bf16_valued(gen("normal_f32", 25, (37, K)) * 4)).to(torch.bfloat16)
    x = xt.float().numpy()
    for act in packed.ACTS:
        for decode_kernel in packed.MATMUL_MLP_DECODE_KERNELS:
            mlp = packed.PackedMatmulMLP(gate, up, down, act=act, decode_kernel=decode_kernel)
            assert mlp.backend == "emulation" and (mlp.in_features, mlp.hidden_features, mlp.out_features) == (K, N, K_OUT)
            for rows in (37, 7):
                h = _round(_glu64(x[:rows], gate, up, act, None, None), "bfloat16")
                want = _round(_f64(h.float().numpy(), down, None), "bfloat16")
                y = mlp(xt[:rows])
                assert y.dtype == torch.bfloat16 and tuple(y.shape) == (rows, K_OUT) and torch.equal(y.view(torch.int16), want.view(torch.int16))
            assert tuple(mlp(xt[:0]).shape) == (0, K_OUT) and tuple(mlp(xt[:36].reshape(4, 9, K)).shape) == (4, 9, K_OUT)
    count, rows = 3, [0, 5, 5, 21]
    gates, ups, downs = _kn_experts(count)
    for decode_max_rows in (None, 21):
        experts = packed.PackedExpertsMatmulMLP(gates, ups, downs, decode_max_rows=decode_max_rows, out_dtype="float32")
        assert (experts.count, experts.in_features, experts.hidden_features, experts.out_features) == (count, K, N, K_OUT)
        h = _round(_grouped64(x[:21], rows, gates, ups, "silu", None, None), "bfloat16").float().numpy()
        want = np.zeros((21, K_OUT), dtype=np.float64)
        for e in range(count):
            want[rows[e]:rows[e + 1]] = _f64(h[rows[e]:rows[e + 1]], downs[e], None)
        y = experts(xt[:21], rows)
        assert y.dtype == torch.float32 and np.array_equal(y.numpy().view(np.uint32), _round(want).view(np.uint32))
        assert experts._decode_workspace is None and tuple(experts(xt[:0], [0] * (count + 1)).shape) == (0, K_OUT)
    # refusals
    for bad in ("skinny", "auto", None, ""):
        with pytest.raises(hb.MtqError, match="decode_kernel must be one of"):
            packed.PackedMatmulMLP(gate, up, down, decode_kernel=bad)
    with pytest.raises(hb.MtqError, match=rf"down must be a 2-D \({N}, k_out\)"):
        packed.PackedMatmulMLP(gate, up, gate)
    with pytest.raises(hb.MtqError, match="act must be"):
        packed.PackedMatmulMLP(gate, up, down, act="gelu")
    with pytest.raises(hb.MtqError, match="out_dtype"):
        packed.PackedMatmulMLP(gate, up, down, out_dtype="float16")
    with pytest.raises(hb.MtqError, match=rf"x must be \(\.\.\., {K}\)"):
        packed.PackedMatmulMLP(gate, up, down)(xt[:, :N])
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(hb.MtqError, match="decode_max_rows"):
            packed.PackedExpertsMatmulMLP(gates, ups, downs, decode_max_rows=bad)
    with pytest.raises(hb.MtqError, match="as many experts of one shape"):
        packed.PackedExpertsMatmulMLP(gates, ups[:2], downs)
    with pytest.raises(hb.MtqError, match="down batch must hold"):
        packed.PackedExpertsMatmulMLP(gates, ups, gates)


def test_packed_moe_stored_transpose_on_emulation_is_plan_dispatch_experts_combine():
    count, T, topk = 3, 9, 2
    gates, ups, downs = _kn_experts(count)
    rng = np.random.default_rng(5)
    xt = torch.from_numpy(to_bf16_valued(gen("normal_f32", 61, (T, K)) * 4)).to(torch.bfloat16)
    x = xt.float().numpy()
    ids = rng.integers(-1, count + 1, size=(T, topk)).astype(np.int64)            # -1 and count are dropped
    ids[0] = [1, 1]                                                               # a token that names one expert twice
    assert (ids < 0).any() and (ids >= count).any()
    w = (rng.random((T, topk)) + 0.25).astype(np.float32)
    base = to_bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))
    moe = packed.PackedMoE(gates, ups, downs, out_dtype="float32", stored="transpose")
    assert type(moe.experts).__name__ == "PackedExpertsMatmulMLP" and moe.stored == "transpose" and moe.backend == "emulation"
    assert (moe.count, moe.in_features, moe.out_features) == (count, K, K_OUT)
    # plan: the stable sort of the live slots by expert; dispatch: their tokens' rows
    flat = ids.reshape(-1)
    live = [s for e in range(count) for s in range(T * topk) if flat[s] == e]
    group_rows = [0] + list(np.cumsum([int((flat == e).sum()) for e in range(count)]))
    xs = x[[s // topk for s in live]]
    # per expert: glu_matmul into bf16, matmul with the down matrix into float32 (the default expert_dtype)
    ys = np.zeros((len(live), K_OUT), dtype=np.float32)
    for e in range(count):
        r0, r1 = group_rows[e], group_rows[e + 1]
        if r1 > r0:
            h = packed.glu_matmul(xs[r0:r1], gates[e], ups[e], out_dtype="bfloat16")
            ys[r0:r1] = packed.matmul(h, downs[e])
    row_of = {s: r for r, s in enumerate(live)}
    for with_base in (False, True):
        want = (base.copy() if with_base else np.zeros((T, K_OUT), dtype=np.float32))
        for t in range(T):
            for j in range(topk):
                r = row_of.get(t * topk + j)
                if r is not None:
                    want[t] = (want[t] + (w[t, j] * ys[r]).astype(np.float32)).astype(np.float32)
        y = moe(xt, torch.from_numpy(ids), torch.from_numpy(w), base=torch.from_numpy(base) if with_base else None)
        assert y.dtype == torch.float32 and np.array_equal(y.numpy().view(np.uint32), want.view(np.uint32)), with_base
    assert tuple(moe(xt[:0], torch.from_numpy(ids[:0]), torch.from_numpy(w[:0])).shape) == (0, K_OUT)


def test_stored_rows_still_constructs_the_row_layout_experts():
    wg = np.stack([gen("heavy_f32", 30 + i, (N, K)) for i in range(2)])
    wd = np.stack([gen("heavy_f32", 50 + i, (K_OUT, N)) for i in range(2)])
    gates = packed.pack_batch(wg, np.stack([random_map((N, K), 33 + i) for i in range(2)]))
    downs = packed.pack_batch(wd, np.stack([random_map((K_OUT, N), 53 + i) for i in range(2)]))
    for kw in ({}, {"stored": "rows"}):
        moe = packed.PackedMoE(gates, gates, downs, **kw)
        assert type(moe.experts).__name__ == "PackedExpertsMLP" and moe.stored == "rows"
    for bad in ("transposed", "cols", None, ""):
        with pytest.raises(hb.MtqError, match="stored must be one of"):
            packed.PackedMoE(gates, gates, downs, stored=bad)
    with pytest.raises(hb.MtqError):                     # row-layout experts under the other word: the shapes do not fit
        packed.PackedMoE(gates, gates, downs, stored="transpose")


def test_a_store_transposed_directory_of_experts_runs_through_packed_moe(tmp_path):
    """A directory as scripts/pack_model.py --store-transposed writes it (every entry "stored": "transpose", the packed tensor the
    weight's transpose): load_dir, the index's word, PackedMoE - no loop over experts in the caller."""
    count, T, topk = 3, 6, 2
    gates, ups, downs = _kn_experts(count)
    named, meta = {}, {}
    for proj, pts, shape in (("gate_proj", gates, (N, K)), ("up_proj", ups, (N, K)), ("down_proj", downs, (K_OUT, N))):
        for e, pt in enumerate(pts):
            named[f"experts.{e}.{proj}.weight"] = pt
            meta[f"experts.{e}.{proj}.weight"] = {"stored": "transpose", "source_shape": list(shape)}
    packed.save_dir(tmp_path, named, meta=meta, run={"stored": "transpose"})
    index, loaded = packed.read_index(tmp_path), packed.load_dir(tmp_path)
    words = {entry["stored"] for entry in index["tensors"].values()}
    assert words == {"transpose"} and index["run"]["stored"] == "transpose"
    lists = [[loaded[f"experts.{e}.{proj}.weight"] for e in range(count)] for proj in ("gate_proj", "up_proj", "down_proj")]
    moe = packed.PackedMoE(*lists, out_dtype="float32", stored=words.pop())
    xt = torch.from_numpy(to_bf16_valued(gen("normal_f32", 71, (T, K)) * 4)).to(torch.bfloat16)
    ids = torch.from_numpy(np.random.default_rng(3).integers(0, count, size=(T, topk)))
    w = torch.rand((T, topk), generator=torch.Generator().manual_seed(1)) + 0.25
    want = packed.PackedMoE(gates, ups, downs, out_dtype="float32", stored="transpose")(xt, ids, w)
    y = moe(xt, ids, w)
    assert tuple(y.shape) == (T, K_OUT) and torch.equal(y.view(torch.int32), want.view(torch.int32)) and bool(y.abs().max() > 0)
