"""CPU-only: the packed products for (n, k) weights (linear, glu, PackedLinear, ...) and their twins for (k, n) matrices (matmul,
glu_matmul, PackedMatmul, ...), held side by side.  First the emulation of every public pair gives the same bits for the same matrix;
then each point in which the two families differ on the hip route is pinned: which optional symbols a call asks for, what "auto" does
when a constant is None, which of hip_backend's bindings return before the library at m = 0, the tile grid's orientation and wording,
how the modules size their workspaces, and the order in which a bad call's errors are reported.  The hip routes run against
recorders; nothing here needs a device.

The twin of a packed (k, n) matrix P̂ is the all-bf16 packing of unpack(P̂)ᵀ (a BFP group runs along a row of the stored matrix, so
the same map on Wᵀ would quantise other groups).  The inputs lie on a dyadic grid on which every float64 sum is exact, so the two
products agree whatever order they are summed in."""
import types

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.packed_cases import GRID, random_map, uniform_map
from tests.test_capi_host import _load, _OnDevice, _StubLibrary

N, K, KOUT, COUNT = 40, 72, 48, 3          # 2 x 3 tiles with partial edges; the down projection (KOUT, N)
MS = (0, 1, 32, 33)
GROUP_ROWS = [0, 2, 2, 5]                  # three groups, the middle one empty


def _grid(seed, shape, lim=255):
    return (np.random.default_rng(seed).integers(-lim, lim + 1, size=shape) * GRID).astype(np.float32)


def _x(m, k=K, seed=7):
    return np.random.default_rng(seed + m).integers(-4, 5, size=(m, k)).astype(np.float32)


def _pair(seed, n=N, k=K):
    """(the (n, k) tensor, its (k, n) twin): a mixed map on the (k, n) side, the all-bf16 packing of its transpose on the other."""
    kn = packed.pack_transposed(_grid(seed, (n, k)), random_map((k, n), seed))
    w = packed.unpack_transposed(kn)
    nk = packed.pack(w, uniform_map((n, k), 0))
    assert np.array_equal(packed.unpack(nk).view(np.uint32), w.view(np.uint32))
    return nk, kn


def _batch_pair(seed, n=N, k=K):
    w3 = _grid(seed, (COUNT, n, k))
    maps = np.stack([random_map((k, n), seed + i) for i in range(COUNT)])
    kn = packed.pack_batch_transposed(w3, maps)
    nk = packed.pack_batch(packed.unpack_batch_transposed(kn), np.zeros((COUNT, -(-n // 32), -(-k // 32)), dtype=np.int8))
    return nk, kn


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                                                                            b.view(np.uint32 if b.dtype == np.float32 else np.uint64))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                                                      b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def test_every_public_pair_gives_the_same_bits_on_the_emulation():
    (g_nk, g_kn), (u_nk, u_kn), (d_nk, d_kn) = _pair(1), _pair(2), _pair(3, KOUT, N)
    (gb_nk, gb_kn), (ub_nk, ub_kn), (db_nk, db_kn) = _batch_pair(4), _batch_pair(5), _batch_pair(6, KOUT, N)
    b, b2, bc, bc2 = _grid(8, (N,)), _grid(9, (N,)), _grid(10, (COUNT, N)), _grid(11, (COUNT, N))
    xg = _x(GROUP_ROWS[-1])
    x3 = _x(COUNT * 4).reshape(COUNT, 4, K)
    checked = 0

    def pair(name_nk, name_kn, args_nk, args_kn, **kw):
        nonlocal checked
        got_nk, got_kn = getattr(packed, name_nk)(*args_nk, **kw), getattr(packed, name_kn)(*args_kn, **kw)
        assert _same(got_nk, got_kn), (name_nk, name_kn, kw)
        checked += 1
        return got_nk

    for out_dtype in ("float32", "bfloat16"):
        for bias in (None, b):
            for m in MS:
                x = _x(m)
                for kernel in packed.KERNELS:
                    y = pair("linear", "matmul", (x, g_nk), (x, g_kn), bias=bias, out_dtype=out_dtype, kernel=kernel)
                    assert tuple(y.shape) == (m, N)
                pair("linear_wide", "matmul_wide", (x, g_nk), (x, g_kn), bias=bias, out_dtype=out_dtype)
                for kernel in packed.GLU_KERNELS:
                    pair("glu", "glu_matmul", (x, g_nk, u_nk), (x, g_kn, u_kn), bias_gate=bias, bias_up=None if bias is None else b2,
                         out_dtype=out_dtype, kernel=kernel)
                pair("glu_skinny", "glu_matmul_skinny", (x, g_nk, u_nk), (x, g_kn, u_kn), act="none", bias_gate=bias, out_dtype=out_dtype, split=2)
        for bias in (None, bc):
            for kernel in packed.GROUPED_KERNELS:
                pair("linear_grouped", "matmul_grouped", (xg, GROUP_ROWS, gb_nk), (xg, GROUP_ROWS, gb_kn), bias=bias, out_dtype=out_dtype, kernel=kernel)
                pair("linear_batch", "matmul_batch", (x3, gb_nk), (x3, gb_kn), bias=bias, out_dtype=out_dtype, kernel=kernel)
            pair("linear_grouped_wide", "matmul_grouped_wide", (xg, GROUP_ROWS, gb_nk), (xg, GROUP_ROWS, gb_kn), bias=bias, out_dtype=out_dtype)
            for kernel in packed.GLU_GROUPED_KERNELS:
                pair("glu_grouped", "glu_matmul_grouped", (xg, GROUP_ROWS, gb_nk, ub_nk), (xg, GROUP_ROWS, gb_kn, ub_kn), bias_gate=bias,
                     bias_up=None if bias is None else bc2, out_dtype=out_dtype, kernel=kernel)
            pair("glu_grouped_skinny", "glu_matmul_grouped_skinny", (xg, GROUP_ROWS, gb_nk, ub_nk), (xg, GROUP_ROWS, gb_kn, ub_kn), bias_up=bias,
                 out_dtype=out_dtype)
    for act in packed.ACTS:
        h = pair("glu_emulation_f64", "glu_matmul_emulation_f64", (xg, g_nk, u_nk), (xg, g_kn, u_kn), act=act, bias_gate=b, bias_up=b2)
        assert h.dtype == np.float64
    # the same pairs with an empty x, a device-less torch group_rows and one host bias among the grouped calls
    pair("linear_grouped", "matmul_grouped", (xg[:0], [0, 0, 0, 0], gb_nk), (xg[:0], [0, 0, 0, 0], gb_kn))
    pair("linear_grouped", "matmul_grouped", (xg, torch.tensor(GROUP_ROWS), gb_nk), (xg, torch.tensor(GROUP_ROWS), gb_kn), bias=torch.from_numpy(bc))
    # the modules: same constructor keywords (the positional order of backend and kernel differs between PackedLinear and PackedMatmul)
    xt = torch.from_numpy(_x(6).reshape(2, 3, K)).to(torch.bfloat16)
    xgt = torch.from_numpy(xg).to(torch.bfloat16)

    def modules(name_nk, name_kn, args_nk, args_kn, call, **kw):
        nonlocal checked
        a, c = getattr(packed, name_nk)(*args_nk, **kw), getattr(packed, name_kn)(*args_kn, **kw)
        assert a.backend == c.backend == "emulation"
        assert (a.in_features, a.out_features) == (c.in_features, c.out_features)
        assert a.extra_repr() == c.extra_repr()                                  # packed_bytes apart, see below
        assert _same(a(*call), c(*call)), (name_nk, kw)
        checked += 1

    for out_dtype in ("float32", "bfloat16"):
        modules("PackedExperts", "PackedExpertsMatmul", (gb_nk,), (gb_kn,), (xgt, GROUP_ROWS), bias=bc, out_dtype=out_dtype, kernel="auto", wide_min_rows=4)
        modules("PackedMLP", "PackedMatmulMLP", (g_nk, u_nk, d_nk), (g_kn, u_kn, d_kn), (xt,), out_dtype=out_dtype, decode_kernel="fused")
        for rows in (None, 8):
            modules("PackedExpertsMLP", "PackedExpertsMatmulMLP", (gb_nk, ub_nk, db_nk), (gb_kn, ub_kn, db_kn), (xgt, GROUP_ROWS), out_dtype=out_dtype,
                    decode_max_rows=rows)
        lin, mat = packed.PackedLinear(g_nk, bias=b, out_dtype=out_dtype), packed.PackedMatmul(g_kn, bias=b, out_dtype=out_dtype)
        assert (lin.kernel, mat.kernel) == ("auto", "block")                     # the defaults differ
        assert (lin.in_features, lin.out_features) == (mat.in_features, mat.out_features) == (K, N) and _same(lin(xt), mat(xt))
        ids = torch.tensor([[0, 2], [1, 5], [2, 2], [0, 1]])
        wts = torch.from_numpy(_grid(12, (4, 2)))
        x4 = torch.from_numpy(_x(4)).to(torch.bfloat16)
        moe_nk = packed.PackedMoE(gb_nk, ub_nk, db_nk, out_dtype=out_dtype)
        moe_kn = packed.PackedMoE(gb_kn, ub_kn, db_kn, out_dtype=out_dtype, stored="transpose")
        assert type(moe_nk.experts) is packed.PackedExpertsMLP and type(moe_kn.experts) is packed.PackedExpertsMatmulMLP
        assert _same(moe_nk(x4, ids, wts), moe_kn(x4, ids, wts))
        checked += 2
    assert checked > 150


# ----------------------------------------------------------------------------- the hip route of packed.py against recorders

DATA = torch.zeros(1, dtype=torch.uint8)           # stands for a device stream: no recorder reads it
SINGLE = ("packed_linear", "packed_linear_wide", "packed_linear_skinny", "packed_matmul", "packed_matmul_wide", "packed_matmul_skinny")
GATED = ("packed_glu_wide", "packed_glu_skinny", "packed_glu_matmul_wide", "packed_glu_matmul_skinny")


def _record_single(monkeypatch, calls):
    """Every single-tensor binding of hip_backend replaced by a recorder of (its name, m, its keywords) that returns zeros (m, n)."""
    monkeypatch.setattr(packed, "_device_data", lambda p: DATA)
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")

    def plain(name):
        def record(x, data, tables, n, **kw):
            assert data is DATA and tables == "tables"
            calls.append((name, int(x.shape[0]), n, dict(kw)))
            return torch.zeros((int(x.shape[0]), n))
        return record

    def gated(name):
        def record(x, gd, gt, ud, ut, n, **kw):
            calls.append((name, int(x.shape[0]), n, dict(kw)))
            return torch.zeros((int(x.shape[0]), n))
        return record

    for name in SINGLE:
        monkeypatch.setattr(hb, name, plain(name))
    for name in GATED:
        monkeypatch.setattr(hb, name, gated(name))
    monkeypatch.setattr(hb, "glu_combine", lambda g, u, **kw: calls.append(("glu_combine", int(g.shape[0]), int(g.shape[1]), dict(kw))) or g)


def _names(calls):
    return [c[0] for c in calls]


def _xb(m, k=K):
    return torch.zeros((m, k), dtype=torch.bfloat16)


def _message(fn, *args, **kw):
    with pytest.raises(hb.MtqError) as info:
        fn(*args, **kw)
    return str(info.value)


def test_linear_asks_for_no_optional_symbol_and_matmul_for_its_own_on_every_call(monkeypatch):
    stub = _StubLibrary(143, missing=hb.OPTIONAL_EXPORTS)
    assert _load(monkeypatch, stub) is stub
    (nk, kn), calls = _pair(1), []
    _record_single(monkeypatch, calls)
    for m, kernel, want in ((1, "block", "packed_linear"), (33, "block", "packed_linear"), (1, "skinny", "packed_linear_skinny"),
                            (32, "auto", "packed_linear_skinny"), (33, "auto", "packed_linear"), (300, "auto", "packed_linear")):
        calls.clear()
        packed.linear(_xb(m), nk, backend="hip", kernel=kernel)
        assert _names(calls) == [want], (m, kernel)
    calls.clear()
    packed.linear_wide(_xb(5), nk, backend="hip")                                # no has_ check of its own: the binding is reached
    assert _names(calls) == ["packed_linear_wide"]
    calls.clear()
    for kernel in packed.MATMUL_KERNELS:
        assert _message(packed.matmul, _xb(1), kn, backend="hip", kernel=kernel) == \
            "matmul needs mtq_pack_tiles_transposed, mtq_unpack_tiles_transposed and mtq_packed_matmul, which this build of libmtq_hip.so " \
            "lacks: rebuild it from this tree"
    assert _message(packed.matmul_wide, _xb(1), kn, backend="hip") == \
        "matmul_wide needs mtq_packed_matmul_wide, which this build of libmtq_hip.so lacks: rebuild it from this tree"
    assert _message(packed.PackedMatmul, kn, backend="hip").startswith("PackedMatmul needs mtq_pack_tiles_transposed")
    assert not calls
    # only the skinny symbols missing: the explicit name raises naming them, "auto" goes to the block entry, the module keeps no workspace
    stub = _StubLibrary(143, missing=hb.PACKED_MATMUL_SKINNY)
    assert _load(monkeypatch, stub) is stub
    skinny_lacks = " needs mtq_packed_matmul_skinny_workspace_bytes and mtq_packed_matmul_skinny, which this build of libmtq_hip.so lacks: " \
                   "rebuild it from this tree"
    assert _message(packed.matmul, _xb(1), kn, backend="hip", kernel="skinny") == 'matmul(kernel="skinny")' + skinny_lacks
    assert _message(packed.PackedMatmul, kn, backend="hip", kernel="skinny") == 'PackedMatmul(kernel="skinny")' + skinny_lacks
    assert _message(packed.glu_matmul, _xb(1), kn, kn, backend="hip", kernel="auto") == 'glu_matmul(kernel="auto")' + skinny_lacks
    assert "takes m <= 32, got m = 33" in _message(packed.matmul, _xb(33), kn, backend="hip", kernel="skinny")   # m before the symbol
    packed.matmul(_xb(1), kn, backend="hip", kernel="auto")
    mod = packed.PackedMatmul(kn, backend="hip", kernel="auto")
    assert mod._workspace is None
    mod(_xb(1))
    assert _names(calls) == ["packed_matmul", "packed_matmul"] and sorted(calls[1][3]) == ["bias", "out_dtype"]


def test_auto_gates_and_their_none_values(monkeypatch):
    stub = _StubLibrary(143)
    assert _load(monkeypatch, stub) is stub
    (nk, kn), calls = _pair(1), []
    _record_single(monkeypatch, calls)

    def routed(fn, pt, m, **kw):
        calls.clear()
        fn(_xb(m), *pt, backend="hip", kernel="auto", **kw)
        return _names(calls)

    assert routed(packed.linear, (nk,), 32) == ["packed_linear_skinny"] and routed(packed.linear, (nk,), 33) == ["packed_linear"]
    assert routed(packed.linear, (nk,), 64) == ["packed_linear_wide"]
    assert routed(packed.matmul, (kn,), 32) == ["packed_matmul_skinny"] and routed(packed.matmul, (kn,), 33) == ["packed_matmul"]
    assert routed(packed.matmul, (kn,), 64) == ["packed_matmul_wide"]
    monkeypatch.setattr(packed, "AUTO_WIDE_MIN_M", None)
    monkeypatch.setattr(packed, "AUTO_MATMUL_WIDE_MIN_M", None)
    assert routed(packed.linear, (nk,), 300) == ["packed_linear"] and routed(packed.matmul, (kn,), 300) == ["packed_matmul"]
    monkeypatch.setattr(packed, "AUTO_MATMUL_SKINNY_MAX_M", None)                # the (k, n) side's skinny gate may be None
    assert routed(packed.matmul, (kn,), 1) == ["packed_matmul"]
    monkeypatch.setattr(packed, "AUTO_SKINNY_MAX_M", 4)                          # the (n, k) side's is a number, compared unconditionally
    assert routed(packed.linear, (nk,), 4) == ["packed_linear_skinny"] and routed(packed.linear, (nk,), 5) == ["packed_linear"]
    # the gated product: glu reads AUTO_SKINNY_MAX_M and AUTO_GLU_FUSED_MIN_M, glu_matmul its own two, either of which may be None
    assert routed(packed.glu, (nk, nk), 4) == ["packed_linear_skinny"] * 2 + ["glu_combine"]
    assert routed(packed.glu, (nk, nk), 5) == ["packed_linear"] * 2 + ["glu_combine"]
    assert routed(packed.glu, (nk, nk), 64) == ["packed_glu_wide"]
    assert routed(packed.glu_matmul, (kn, kn), 32) == ["packed_matmul_skinny"] * 2 + ["glu_combine"]
    assert routed(packed.glu_matmul, (kn, kn), 33) == ["packed_matmul"] * 2 + ["glu_combine"]
    assert routed(packed.glu_matmul, (kn, kn), 64) == ["packed_glu_matmul_wide"]
    monkeypatch.setattr(packed, "AUTO_GLU_MATMUL_SKINNY_MAX_M", None)
    monkeypatch.setattr(packed, "AUTO_GLU_MATMUL_FUSED_MIN_M", None)
    monkeypatch.setattr(packed, "AUTO_GLU_FUSED_MIN_M", None)
    assert routed(packed.glu_matmul, (kn, kn), 1) == ["packed_matmul"] * 2 + ["glu_combine"]
    assert routed(packed.glu_matmul, (kn, kn), 300) == ["packed_matmul"] * 2 + ["glu_combine"]
    assert routed(packed.glu, (nk, nk), 300) == ["packed_linear"] * 2 + ["glu_combine"]
    # the dense MLP modules compare against the same constants: PackedMLP AUTO_SKINNY_MAX_M, PackedMatmulMLP AUTO_GLU_MATMUL_SKINNY_MAX_M
    d_nk, d_kn = _pair(3, KOUT, N)
    mlp = packed.PackedMLP(nk, nk, d_nk, backend="hip", decode_kernel="fused")
    mlp_kn = packed.PackedMatmulMLP(kn, kn, d_kn, backend="hip", decode_kernel="fused")
    for mod, m, want in ((mlp, 4, "packed_glu_skinny"), (mlp, 5, "packed_linear"), (mlp_kn, 1, "packed_matmul")):
        calls.clear()
        assert tuple(mod(_xb(m)).shape) == (m, KOUT) and calls[0][0] == want, (m, want)
    monkeypatch.setattr(packed, "AUTO_GLU_MATMUL_SKINNY_MAX_M", 2)
    for m, want in ((2, "packed_glu_matmul_skinny"), (3, "packed_matmul")):
        calls.clear()
        mlp_kn(_xb(m))
        assert calls[0][0] == want


def test_the_order_of_checks_of_a_bad_call(monkeypatch):
    """kernel name → shape → backend → out_dtype → x shape → missing symbol, per public function as it stands."""
    stub = _StubLibrary(143, missing=hb.OPTIONAL_EXPORTS)
    assert _load(monkeypatch, stub) is stub
    (nk, kn) = _pair(1)
    nk3 = packed.pack(_grid(1, (2, 32, 64)), uniform_map((64, 64), 0))
    bad_x = _xb(1, K + 1)
    assert "kernel must be one of ('block', 'skinny', 'auto')" in _message(packed.linear, bad_x, nk3, kernel="x", out_dtype="f", backend="b")
    assert _message(packed.linear, bad_x, nk3, out_dtype="f", backend="b") == "linear needs a 2-D (n, k) weight, the packed tensor is (2, 32, 64)"
    assert _message(packed.linear, bad_x, nk, out_dtype="f", backend="b") == "out_dtype must be 'float32' or 'bfloat16', got 'f'"
    assert _message(packed.linear, bad_x, nk, backend="b") == "backend must be one of ('hip', 'emulation'), got 'b'"
    assert _message(packed.linear, bad_x, nk, backend="hip") == f"x must be (m, {K}), got (1, {K + 1})"
    # matmul: the shape before the kernel name
    assert _message(packed.matmul, bad_x, nk3, kernel="x", out_dtype="f") == "matmul needs a 2-D packed (k, n) matrix, the packed tensor is (2, 32, 64)"
    assert "kernel must be one of" in _message(packed.matmul, bad_x, kn, kernel="x", out_dtype="f")
    assert _message(packed.matmul, bad_x, kn, out_dtype="f", backend="hip") == "out_dtype must be 'float32' or 'bfloat16', got 'f'"
    assert _message(packed.matmul, bad_x, kn, backend="hip") == f"x must be (m, {K}), got (1, {K + 1})"          # before the missing symbol
    assert "lacks" in _message(packed.matmul, _xb(1), kn, backend="hip")
    assert _message(packed.matmul_wide, bad_x, kn, backend="hip") == f"x must be (m, {K}), got (1, {K + 1})"
    # the gated pair: weights, act, kernel, out_dtype, then x, then the symbols
    assert _message(packed.glu, bad_x, nk3, nk, act="a") == "glu needs 2-D (n, k) weights, the packed gate tensor is (2, 32, 64)"
    assert _message(packed.glu_matmul, bad_x, nk3, kn, act="a") == "glu_matmul needs a 2-D packed (k, n) matrix, the packed tensor is (2, 32, 64)"
    assert _message(packed.glu_matmul_skinny, bad_x, nk3, kn) == "glu_matmul_skinny needs a 2-D packed (k, n) matrix, the packed tensor is (2, 32, 64)"
    for fn, pt in ((packed.glu, nk), (packed.glu_matmul, kn)):
        assert "act must be one of" in _message(fn, bad_x, pt, pt, act="a", kernel="x")
        assert "kernel must be one of ('fused', 'unfused', 'auto')" in _message(fn, bad_x, pt, pt, kernel="x", out_dtype="f")
        assert "out_dtype" in _message(fn, bad_x, pt, pt, out_dtype="f", backend="hip")
        assert _message(fn, bad_x, pt, pt, backend="hip") == f"x must be (m, {K}), got (1, {K + 1})"
        assert _message(fn, bad_x, pt, pt, backend="b") == "backend must be one of ('hip', 'emulation'), got 'b'"
    assert _message(packed.glu, _xb(1), nk, nk, backend="hip").startswith("glu needs mtq_glu_combine, mtq_packed_glu_wide and")
    assert _message(packed.glu_matmul, _xb(1), kn, kn, backend="hip").startswith("glu_matmul needs mtq_pack_tiles_transposed")
    assert _message(packed.glu_skinny, _xb(33), nk, nk, backend="hip").startswith("glu_skinny needs mtq_packed_glu_skinny and")   # symbol before m
    assert _message(packed.glu_matmul_skinny, _xb(33), kn, kn, backend="hip").startswith("glu_matmul_skinny needs mtq_packed_glu_matmul_skinny_workspace_bytes")
    stub = _StubLibrary(143)
    assert _load(monkeypatch, stub) is stub
    assert _message(packed.glu_skinny, _xb(33), nk, nk, backend="hip") == 'glu_skinny takes m <= 32, got m = 33: glu(kernel="auto") serves every m'
    assert _message(packed.glu_matmul_skinny, _xb(33), kn, kn, backend="hip") == \
        'glu_matmul_skinny takes m <= 32, got m = 33: glu_matmul(kernel="auto") serves every m'


def _record_grouped(monkeypatch, calls):
    monkeypatch.setattr(packed, "batch_to_device", lambda b, device="cuda": packed.PackedBatch(
        b.count, b.rows, b.cols, torch.zeros(1, dtype=torch.uint8), b.bases, "maps", "offsets", "bases", maps=b.maps))

    def plain(name):
        def record(x, group_rows, arena, maps_dev, offsets_dev, bases_dev, count, n, **kw):
            assert (maps_dev, offsets_dev, bases_dev) == ("maps", "offsets", "bases") and group_rows.dtype == torch.int32
            calls.append((name, int(x.shape[0]), count, n, sorted(kw)))
            return torch.zeros((int(x.shape[0]), n))
        return record

    def gated(name):
        def record(x, group_rows, gate, up, count, n, **kw):
            assert gate[1:] == up[1:] == ("maps", "offsets", "bases")
            calls.append((name, int(x.shape[0]), count, n, sorted(kw)))
            return torch.zeros((int(x.shape[0]), n))
        return record

    for fam in ("linear", "matmul"):
        for tail in ("skinny_grouped", "skinny_grouped_chunked", "wide_grouped"):
            monkeypatch.setattr(hb, f"packed_{fam}_{tail}", plain(f"packed_{fam}_{tail}"))
    for fam in ("glu", "glu_matmul"):
        for tail in ("wide_grouped", "skinny_grouped"):
            monkeypatch.setattr(hb, f"packed_{fam}_{tail}", gated(f"packed_{fam}_{tail}"))
    monkeypatch.setattr(hb, "glu_combine", lambda g, u, **kw: calls.append(("glu_combine", int(g.shape[0]), None, int(g.shape[1]), sorted(kw))) or g)


def test_grouped_routes_and_which_of_them_check_for_their_symbols(monkeypatch):
    stub = _StubLibrary(143)
    assert _load(monkeypatch, stub) is stub
    (nk, kn), (up_nk, up_kn), calls = _batch_pair(4), _batch_pair(5), []
    nk, kn, up_nk, up_kn = (packed.as_batch(b) for b in (nk, kn, up_nk, up_kn))
    _record_grouped(monkeypatch, calls)
    xg = _xb(5)
    with_split, no_split = ["bias", "out_dtype", "split", "workspace"], ["bias", "out_dtype", "workspace"]
    for fam, fn, wide, batch in (("linear", packed.linear_grouped, packed.linear_grouped_wide, nk),
                                 ("matmul", packed.matmul_grouped, packed.matmul_grouped_wide, kn)):
        for kernel, tail in (("walk", "skinny_grouped"), ("chunks", "skinny_grouped_chunked"), ("auto", "skinny_grouped_chunked")):
            calls.clear()
            assert tuple(fn(xg, GROUP_ROWS, batch, backend="hip", kernel=kernel).shape) == (5, N)
            assert calls == [(f"packed_{fam}_{tail}", 5, COUNT, N, with_split)]
        calls.clear()
        wide(xg, GROUP_ROWS, batch, backend="hip")
        assert calls == [(f"packed_{fam}_wide_grouped", 5, COUNT, N, no_split)]
        calls.clear()
        assert tuple(fn(xg[:0], [0, 0, 0, 0], batch, backend="hip", out_dtype="bfloat16").shape) == (0, N) and not calls     # T = 0: no call
        assert tuple(wide(xg[:0], [0, 0, 0, 0], batch, backend="hip").shape) == (0, N) and not calls
    gated_kw = ["act", "bias_gate", "bias_up", "out_dtype", "workspace"]
    for fam, lin, fn, fn_skinny, g, u in (("glu", "linear", packed.glu_grouped, packed.glu_grouped_skinny, nk, up_nk),
                                          ("glu_matmul", "matmul", packed.glu_matmul_grouped, packed.glu_matmul_grouped_skinny, kn, up_kn)):
        calls.clear()
        fn(xg, GROUP_ROWS, g, u, backend="hip")
        fn_skinny(xg, GROUP_ROWS, g, u, backend="hip")
        fn(xg, GROUP_ROWS, g, u, backend="hip", kernel="unfused")
        assert calls == [(f"packed_{fam}_wide_grouped", 5, COUNT, N, gated_kw), (f"packed_{fam}_skinny_grouped", 5, COUNT, N, sorted(gated_kw + ["split"])),
                         (f"packed_{lin}_wide_grouped", 5, COUNT, N, no_split), (f"packed_{lin}_wide_grouped", 5, COUNT, N, no_split),
                         ("glu_combine", 5, None, N, ["act", "out_dtype"])]
    # a library without the optional symbols: the (n, k) walk is reached all the same, every other grouped route raises before device work
    stub = _StubLibrary(143, missing=hb.OPTIONAL_EXPORTS)
    assert _load(monkeypatch, stub) is stub
    calls.clear()
    packed.linear_grouped(xg, GROUP_ROWS, nk, backend="hip", kernel="walk")
    assert tuple(packed.PackedExperts(nk, backend="hip", kernel="walk")(xg[:0], torch.tensor([0, 0, 0, 0])).shape) == (0, N)   # the constructor asks for nothing
    assert _names(calls) == ["packed_linear_skinny_grouped"]
    calls.clear()
    assert _message(packed.linear_grouped, xg, GROUP_ROWS, nk, backend="hip", kernel="chunks") == \
        'kernel="chunks" needs mtq_packed_linear_skinny_grouped_chunked, which this build of libmtq_hip.so lacks: rebuild it from this tree, ' \
        'or use kernel="walk"'
    assert _message(packed.linear_grouped_wide, xg, GROUP_ROWS, nk, backend="hip") == \
        "linear_grouped_wide needs mtq_packed_linear_wide_grouped, which this build of libmtq_hip.so lacks: rebuild it from this tree, or use " \
        "linear_grouped"
    lacks = ", which this build of libmtq_hip.so lacks: rebuild it from this tree"
    for kernel, names in (("walk", hb.MATMUL_GROUPED), ("chunks", hb.MATMUL_GROUPED_CHUNKED)):
        assert _message(packed.matmul_grouped, xg, GROUP_ROWS, kn, backend="hip", kernel=kernel) == \
            f'matmul_grouped(kernel="{kernel}") needs {" and ".join(names)}' + lacks
        assert _message(packed.PackedExpertsMatmul, kn, backend="hip", kernel=kernel) == f'matmul_grouped(kernel="{kernel}") needs {" and ".join(names)}' + lacks
    assert _message(packed.matmul_grouped_wide, xg, GROUP_ROWS, kn, backend="hip") == \
        f'matmul_grouped_wide needs {" and ".join(hb.MATMUL_WIDE_GROUPED)}' + lacks
    assert _message(packed.glu_grouped, xg, GROUP_ROWS, nk, up_nk, backend="hip").startswith("glu_grouped needs mtq_glu_combine, mtq_packed_glu_wide and")
    assert _message(packed.glu_grouped_skinny, xg, GROUP_ROWS, nk, up_nk, backend="hip").startswith("glu_grouped_skinny needs mtq_packed_glu_skinny and")
    assert _message(packed.glu_matmul_grouped, xg, GROUP_ROWS, kn, up_kn, backend="hip") == \
        f'glu_matmul_grouped needs mtq_glu_combine and {" and ".join(hb.PACKED_GLU_MATMUL)}' + lacks
    assert _message(packed.glu_matmul_grouped_skinny, xg, GROUP_ROWS, kn, up_kn, backend="hip") == \
        f'glu_matmul_grouped_skinny needs {" and ".join(hb.PACKED_GLU_MATMUL_SKINNY)}' + lacks
    assert _message(packed.PackedExpertsMLP, nk, up_nk, nk, backend="hip").startswith("the down batch must hold")     # shapes before symbols
    assert not calls


def test_the_modules_size_their_workspaces_each_in_its_own_way(monkeypatch):
    stub = _StubLibrary(143)
    assert _load(monkeypatch, stub) is stub
    (nk, kn), sized = _pair(1), []
    monkeypatch.setattr(packed, "_device_data", lambda p: DATA)
    monkeypatch.setattr(packed.PackedTensor, "tables", lambda self: "tables")
    monkeypatch.setattr(hb, "packed_linear_skinny_workspace_bytes", lambda m, n, k, split=0: sized.append(("linear", m, n, k)) or 16 * m)
    monkeypatch.setattr(hb, "packed_matmul_skinny_workspace_bytes", lambda m, n, k, split=0: sized.append(("matmul", m, n, k)) or 16 * m)
    lin = packed.PackedLinear(nk, backend="hip")
    assert sized == [("linear", m, N, K) for m in range(1, 33)] and lin._workspace.numel() == 16 * 32     # the maximum over m = 1 .. 32
    sized.clear()
    mat = packed.PackedMatmul(kn, backend="hip", kernel="auto")
    assert sized == [("matmul", 32, N, K)] and mat._workspace.numel() == 16 * 32                          # m = 32 alone
    sized.clear()
    assert packed.PackedLinear(nk, backend="hip", kernel="block")._workspace is None and packed.PackedMatmul(kn, backend="hip")._workspace is None
    assert not sized
    # the grouped modules: PackedExperts looks its size function up at every forward, PackedExpertsMatmul keeps the one it found
    (bnk, bkn), calls = _batch_pair(4), []
    bnk, bkn = packed.as_batch(bnk), packed.as_batch(bkn)
    _record_grouped(monkeypatch, calls)
    for fam in ("linear", "matmul"):
        monkeypatch.setattr(hb, f"packed_{fam}_skinny_grouped_workspace_bytes", lambda T, c, n, k, split=0, fam=fam: sized.append((fam, "early", T, c, n, k, split)) or 32)
        monkeypatch.setattr(hb, f"packed_{fam}_wide_grouped_workspace_bytes", lambda T, c, n, k, fam=fam: sized.append((fam, "wide", T, c, n, k)) or 48)
    experts = packed.PackedExperts(bnk, backend="hip", split=2, wide_min_rows=100)
    experts_kn = packed.PackedExpertsMatmul(bkn, backend="hip", split=2, wide_min_rows=100)
    assert sized == [("linear", "wide", 1, COUNT, N, K), ("matmul", "wide", 1, COUNT, N, K)]
    assert experts._workspace.numel() == experts_kn._workspace.numel() == 48
    for fam in ("linear", "matmul"):
        monkeypatch.setattr(hb, f"packed_{fam}_skinny_grouped_workspace_bytes", lambda T, c, n, k, split=0, fam=fam: sized.append((fam, "late", T, c, n, k, split)) or 64)
    sized.clear()
    experts(_xb(5), torch.tensor(GROUP_ROWS))
    experts_kn(_xb(5), torch.tensor(GROUP_ROWS))
    assert sized == [("linear", "late", 5, COUNT, N, K, 2), ("matmul", "early", 5, COUNT, N, K, 2)]
    assert (experts._workspace.numel(), experts_kn._workspace.numel()) == (64, 48)
    assert _names(calls) == ["packed_linear_skinny_grouped", "packed_matmul_skinny_grouped"]


# ----------------------------------------------------------------------------- hip_backend's bindings against a recording library

class _Entries:
    """Stands for hip_backend._entry: every C entry is a recorder of (name, arguments); a size function answers `size`."""

    def __init__(self, size=0):
        self.calls, self.size = [], size

    def __call__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.size if name.endswith("_workspace_bytes") else 0
        return fn


def _dev(*shape, dtype=torch.bfloat16):
    return _OnDevice(torch.zeros(shape, dtype=dtype))


def _tables(rows, cols):
    th, tw = hb.tiles_hw(rows, cols)
    return types.SimpleNamespace(tiles_h=th, tiles_w=tw, nbytes=320 * th * tw, map_ptr=11, offsets_ptr=12)


@pytest.fixture
def entries(monkeypatch):
    e = _Entries()
    monkeypatch.setattr(hb, "_entry", e)
    monkeypatch.setattr(hb, "require_gpu", lambda: None)
    return e


def test_single_tensor_bindings_pass_the_same_arguments_and_differ_at_m_0_and_in_the_grid(entries):
    data = _dev(1 << 16, dtype=torch.uint8)
    bias = _dev(N, dtype=torch.float32)
    for fam, rows_cols, noun in (("linear", (N, K), f"a {N}x{K} weight"), ("matmul", (K, N), f"a {K}x{N} matrix")):
        tables = _tables(*rows_cols)
        head = lambda m, b: (0, m, K, K, 0, tables.nbytes, 11, 12, N, b, 0, hb.DTYPE_F32, N)     # x, m, k, ldx, stream, bytes, map, offsets, n, bias, y, code, ldy
        for m in (1, 33):
            for tail in ("", "_wide"):
                entries.calls.clear()
                out = _dev(m, N, dtype=torch.float32)
                assert getattr(hb, f"packed_{fam}{tail}")(_dev(m, K), data, tables, N, bias=bias, out=out, stream=None) is out
                assert entries.calls == [(f"mtq_packed_{fam}{tail}", head(m, 0) + (None,))]
        for split, size in ((0, 0), (3, 4096)):
            entries.calls.clear()
            entries.size = size
            ws = None if not size else _dev(size, dtype=torch.uint8)
            getattr(hb, f"packed_{fam}_skinny")(_dev(2, K), data, tables, N, out=_dev(2, N, dtype=torch.float32), split=split, workspace=ws, stream=None)
            assert entries.calls == [(f"mtq_packed_{fam}_skinny_workspace_bytes", (2, N, K, split)),
                                     (f"mtq_packed_{fam}_skinny", head(2, None) + (split, 0 if size else None, size, None))]
        entries.size = 0
        # the grid is read off (n, k) or (k, n), and the message says which
        wrong = _tables(rows_cols[0] + 32, rows_cols[1])
        for tail in ("", "_wide", "_skinny"):
            assert _message(getattr(hb, f"packed_{fam}{tail}"), _dev(1, K), data, wrong, N, stream=None) == \
                f"the map is {wrong.tiles_h}x{wrong.tiles_w} tiles, {noun} has {tables.tiles_h}x{tables.tiles_w}"
        assert "takes m <= 32, got m = 33" in _message(getattr(hb, f"packed_{fam}_skinny"), _dev(33, K), data, tables, N, stream=None)
    # m = 0: packed_linear and packed_linear_skinny go on to the library (whose refusal the caller sees); the other four return the empty out
    out0 = _dev(0, N, dtype=torch.float32)
    for name, tables, reaches in (("packed_linear", _tables(N, K), ["mtq_packed_linear"]), ("packed_linear_wide", _tables(N, K), []),
                                  ("packed_linear_skinny", _tables(N, K), ["mtq_packed_linear_skinny_workspace_bytes", "mtq_packed_linear_skinny"]),
                                  ("packed_matmul", _tables(K, N), []), ("packed_matmul_wide", _tables(K, N), []),
                                  ("packed_matmul_skinny", _tables(K, N), [])):
        entries.calls.clear()
        assert getattr(hb, name)(_dev(0, K), data, tables, N, out=out0, stream=None) is out0
        assert _names(entries.calls) == reaches, name
    # packed_linear_skinny asks for the size before it looks at `out`; packed_matmul_skinny after
    bad_out = _dev(2, N + 1, dtype=torch.float32)
    for fam, tables, reaches in (("linear", _tables(N, K), ["mtq_packed_linear_skinny_workspace_bytes"]), ("matmul", _tables(K, N), [])):
        entries.calls.clear()
        assert "out must be" in _message(getattr(hb, f"packed_{fam}_skinny"), _dev(2, K), data, tables, N, out=bad_out, stream=None)
        assert _names(entries.calls) == reaches


def test_gated_bindings_pass_the_same_arguments_in_both_orientations(entries):
    data = _dev(1 << 16, dtype=torch.uint8)
    bg, bu = _dev(N, dtype=torch.float32), _dev(N, dtype=torch.float32)
    entries.size = 256
    for fam, rows_cols, noun in (("glu", (N, K), f"a {N}x{K} weight"), ("glu_matmul", (K, N), f"a {K}x{N} matrix")):
        t = _tables(*rows_cols)
        head = (0, 5, K, K, 0, t.nbytes, 11, 12, 0, t.nbytes, 11, 12, N, 0, 0, hb.ACT_CODE["none"], 0, hb.DTYPE_BF16, N)
        entries.calls.clear()
        kw = dict(act="none", bias_gate=bg, bias_up=bu, out_dtype=torch.bfloat16, out=_dev(5, N), stream=None)
        getattr(hb, f"packed_{fam}_wide")(_dev(5, K), data, t, data, t, N, **kw)
        getattr(hb, f"packed_{fam}_skinny")(_dev(5, K), data, t, data, t, N, split=2, workspace=_dev(256, dtype=torch.uint8), **kw)
        assert entries.calls == [(f"mtq_packed_{fam}_wide", head + (None,)), (f"mtq_packed_{fam}_skinny_workspace_bytes", (5, N, K, 2)),
                                 (f"mtq_packed_{fam}_skinny", head + (2, 0, 256, None))]
        wrong = _tables(rows_cols[0] + 32, rows_cols[1])
        for tail in ("wide", "skinny"):
            assert _message(getattr(hb, f"packed_{fam}_{tail}"), _dev(1, K), data, t, data, wrong, N, stream=None) == \
                f"the up map is {wrong.tiles_h}x{wrong.tiles_w} tiles, {noun} has {t.tiles_h}x{t.tiles_w}"
            entries.calls.clear()
            out0 = _dev(0, N, dtype=torch.float32)
            assert getattr(hb, f"packed_{fam}_{tail}")(_dev(0, K), data, t, data, t, N, out=out0, stream=None) is out0 and not entries.calls
        assert "takes m <= 32" in _message(getattr(hb, f"packed_{fam}_skinny"), _dev(33, K), data, t, data, t, N, stream=None)
        # the grouped ones: T = 0 returns before the size function; the arguments are the same list in both orientations
        arena = (_dev(COUNT * t.nbytes, dtype=torch.uint8), _dev(COUNT, t.tiles_h * t.tiles_w, dtype=torch.int8),
                 _dev(COUNT, t.tiles_h * t.tiles_w + 1, dtype=torch.int32), _dev(COUNT + 1, dtype=torch.int64))
        rows = _dev(COUNT + 1, dtype=torch.int32)
        side = (0, COUNT * t.nbytes, 0, 0, 0)
        ghead = (0, 5, K, K, 0) + side + side + (COUNT, N, None, None, 0, hb.ACT_CODE["silu"], 0, hb.DTYPE_F32, N)
        entries.calls.clear()
        getattr(hb, f"packed_{fam}_wide_grouped")(_dev(5, K), rows, arena, arena, COUNT, N, out=_dev(5, N, dtype=torch.float32),
                                                  workspace=_dev(256, dtype=torch.uint8), stream=None)
        getattr(hb, f"packed_{fam}_skinny_grouped")(_dev(5, K), rows, arena, arena, COUNT, N, out=_dev(5, N, dtype=torch.float32), split=3,
                                                    workspace=_dev(256, dtype=torch.uint8), stream=None)
        assert entries.calls == [(f"mtq_packed_{fam}_wide_grouped_workspace_bytes", (5, COUNT, N, K)), (f"mtq_packed_{fam}_wide_grouped", ghead + (0, 256, None)),
                                 (f"mtq_packed_{fam}_skinny_grouped_workspace_bytes", (5, COUNT, N, K, 3)),
                                 (f"mtq_packed_{fam}_skinny_grouped", ghead + (3, 0, 256, None))]
        for tail in ("wide_grouped", "skinny_grouped"):
            entries.calls.clear()
            out0 = _dev(0, N, dtype=torch.float32)
            assert getattr(hb, f"packed_{fam}_{tail}")(_dev(0, K), rows, arena, arena, COUNT, N, out=out0, stream=None) is out0 and not entries.calls


def test_every_size_function_turns_the_librarys_refusal_into_an_error(monkeypatch):
    refused = _Entries(size=(1 << 64) - 1)
    monkeypatch.setattr(hb, "_entry", refused)
    monkeypatch.setattr(hb, "lib", lambda: types.SimpleNamespace(mtq_last_error=lambda: b"too large"))
    sizes = [name for name in dir(hb) if name.startswith("packed_") and name.endswith("_workspace_bytes")]
    assert len(sizes) == 14
    for name in sizes:
        args = (5, N, K) if name.count("grouped") == 0 else (5, COUNT, N, K)
        assert _message(getattr(hb, name), *args) == "libmtq_hip error -1: too large", name
        assert refused.calls[-1] == ("mtq_" + name, args + ((0,) if "skinny" in name else ()))


def test_the_has_predicates_answer_for_exactly_their_symbols(monkeypatch):
    groups = {"has_packed_linear_wide": ("mtq_packed_linear_wide",), "has_packed_matmul": hb.PACKED_MATMUL,
              "has_packed_batch_transposed": hb.PACKED_BATCH_TRANSPOSED, "has_packed_matmul_wide": ("mtq_packed_matmul_wide",),
              "has_packed_matmul_skinny": hb.PACKED_MATMUL_SKINNY,
              "has_packed_linear_grouped_chunked": ("mtq_packed_linear_skinny_grouped_chunked", "mtq_packed_linear_skinny_grouped_chunked_workspace_bytes"),
              "has_packed_linear_wide_grouped": hb.WIDE_GROUPED, "has_packed_matmul_grouped": hb.MATMUL_GROUPED,
              "has_packed_matmul_grouped_chunked": hb.MATMUL_GROUPED_CHUNKED, "has_packed_matmul_wide_grouped": hb.MATMUL_WIDE_GROUPED,
              "has_packed_glu": hb.PACKED_GLU, "has_packed_glu_skinny": hb.PACKED_GLU_SKINNY, "has_packed_glu_matmul": hb.PACKED_GLU_MATMUL,
              "has_packed_glu_matmul_skinny": hb.PACKED_GLU_MATMUL_SKINNY, "has_moe": hb.MOE}
    assert sorted(groups) == sorted(name for name in dir(hb) if name.startswith("has_"))
    for has, names in groups.items():
        for gone in names:
            stub = _StubLibrary(143, missing=(gone,))
            assert _load(monkeypatch, stub) is stub
            assert {name: getattr(hb, name)() for name in groups} == {name: gone not in groups[name] for name in groups}, (has, gone)
