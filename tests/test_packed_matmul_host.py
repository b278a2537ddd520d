"""CPU-only: the packed transpose and the (k, n) product (packed.pack_transposed, unpack_transposed, matmul, PackedMatmul) as far as they
go without a device.  The three C entries are declared, optional and exported; a library without them loads and the four Python entries
raise on hip; each C entry refuses bad arguments with MTQ_ERR_INVALID before a device is looked for; the emulation is the row-layout
emulation of the transpose, byte for byte and word for word, and matmul a float64 expression written out here; the command line packs a
map written for --layout transpose with --store-transposed and refuses it without."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps, hip_backend as hb
from quantization_analysis_amd import model_source, packed
from tests.inputs import gen, to_bf16_valued
from tests.packed_cases import expected_bits, random_map, specials, stream_bytes
from tests.test_capi_host import _load, _StubLibrary

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mtq.h"
NEW = ("mtq_pack_tiles_transposed", "mtq_unpack_tiles_transposed", "mtq_packed_matmul")
INVALID, NO_DEVICE = -1, -3


def _aligned():
    buf = np.zeros(1 << 16, dtype=np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: no check may dereference it


def _last():
    return hb.lib().mtq_last_error().decode()


def test_the_entries_are_declared_optional_and_exported():
    text = HEADER.read_text(encoding="utf-8")
    for name in NEW:
        assert len(re.findall(rf"\b{name}\s*\(", text)) == 1, name
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS
        assert getattr(hb.lib(), name) is not None
    assert set(hb.PACKED_MATMUL) == set(NEW) and hb.has_packed_matmul() is True
    assert hb.MTQ_VERSION == 143 and hb.lib().mtq_version() == 143 and packed.FORMAT_VERSION == 1
    # the row-layout entries' parameter lists, one for one
    assert hb.SIGNATURES[NEW[0]][:2] == hb.SIGNATURES["mtq_pack_tiles"][:2]
    assert hb.SIGNATURES[NEW[1]][:2] == hb.SIGNATURES["mtq_unpack_tiles"][:2]
    assert hb.SIGNATURES[NEW[2]][:2] == hb.SIGNATURES["mtq_packed_linear"][:2]
    assert "bit for bit what mtq_packed_linear gives" in text                                     # the bit contract is in the header


def test_a_build_without_the_entries_still_loads(monkeypatch):
    stub = _StubLibrary(143, missing=NEW)
    assert _load(monkeypatch, stub) is stub
    assert stub.mtq_packed_glu_wide.argtypes is not None                        # every other symbol is bound
    assert not hb.has_packed_matmul()
    for name in NEW:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._entry(name)
    w = gen("heavy_f32", 1, (40, 100))
    amap = random_map((100, 40), 2)
    pt = packed.pack_transposed(w, amap)                                        # the emulation needs no library
    x = torch.zeros((5, 100), dtype=torch.bfloat16)
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul.*lacks"):          # no other kernel in their place
        packed.pack_transposed(w, amap, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul.*lacks"):
        packed.unpack_transposed(pt, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul.*lacks"):
        packed.matmul(x, pt, backend="hip")
    with pytest.raises(hb.MtqError, match="mtq_packed_matmul.*lacks"):
        packed.PackedMatmul(pt, backend="hip")


def test_the_transposed_pack_and_unpack_check_their_arguments_before_a_device():
    _buf, p = _aligned()
    big = 1 << 20
    rows, cols = 64, 96                                    # 3 x 2 tiles of the transpose: at least 6 * 320 bytes

    def pack(w=p, dtype=0, rows=rows, cols=cols, ld=cols, amap=p, off=p, out=p, out_bytes=big):
        return hb._entry(NEW[0])(w, dtype, rows, cols, ld, amap, off, out, out_bytes, None)

    def unpack(data=p, nbytes=big, amap=p, off=p, rows=rows, cols=cols, y=p, dtype=1, ldy=cols):
        return hb._entry(NEW[1])(data, nbytes, amap, off, rows, cols, y, dtype, ldy, None)

    def refused(call, match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("w", "amap", "off", "out"):
        refused(pack, "null argument", **{name: None})
    refused(pack, "in_dtype", dtype=7)
    refused(pack, "must be positive", rows=0)
    refused(pack, "must be positive", cols=-1)
    refused(pack, "ld < cols", ld=cols - 1)
    refused(pack, "too large", rows=(1 << 30) + 1)
    refused(pack, "out must be 16-byte aligned", out=p + 8)
    refused(pack, "smaller than the stream", out_bytes=6 * 320 - 1)
    for name in ("data", "amap", "off", "y"):
        refused(unpack, "null argument", **{name: None})
    refused(unpack, "out_dtype", dtype=2)
    refused(unpack, "must be positive", rows=0)
    refused(unpack, "ldy < cols", ldy=cols - 1)
    refused(unpack, "packed must be 16-byte aligned", data=p + 4)
    refused(unpack, "smaller than the stream", nbytes=6 * 320 - 1)
    if not torch.cuda.is_available():                     # everything in order: only the device is missing
        assert pack() == NO_DEVICE and pack(dtype=1, ld=cols + 3) == NO_DEVICE and unpack() == NO_DEVICE and unpack(dtype=0) == NO_DEVICE


def test_matmul_checks_its_arguments_before_a_device():
    fn = hb._entry(NEW[2])
    _buf, p = _aligned()
    m, n, k = 300, 96, 64                                 # 2 x 3 tiles: at least 6 * 320 bytes

    def call(x=p, m=m, k=k, ldx=k, data=p, nbytes=1 << 20, amap=p, off=p, n=n, bias=None, y=p, dtype=hb.DTYPE_F32, ldy=n):
        return fn(x, m, k, ldx, data, nbytes, amap, off, n, bias, y, dtype, ldy, None)

    def refused(match, **kw):
        assert call(**kw) == INVALID, kw
        assert match in _last(), _last()

    for name in ("x", "data", "amap", "off", "y"):
        refused("null argument", **{name: None})
    refused("out_dtype", dtype=5)
    refused("m must be positive", m=0)
    refused("m must be positive", m=-3)
    refused("rows and cols must be positive", n=0)
    refused("rows and cols must be positive", k=0)
    refused("ldx < k", ldx=k - 1)
    refused("ldy < n", ldy=n - 1)
    refused("matrix too large", m=(1 << 40) + 1)
    refused("matrix too large", n=(1 << 30) + 1, ldy=1 << 31)
    refused("packed must be 16-byte aligned", data=p + 8)
    refused("smaller than the stream", nbytes=6 * 320 - 1)
    refused("too many workgroups", m=1 << 40, n=1 << 20, ldy=1 << 20, nbytes=1 << 40)
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE and call(m=1, bias=p, dtype=hb.DTYPE_BF16) == NO_DEVICE


@pytest.mark.parametrize("kind", ["specials", "heavy"])
@pytest.mark.parametrize("n,k", [(40, 100), (72, 300), (1, 17)])
def test_the_emulation_is_the_row_layout_emulation_of_the_transpose(kind, n, k):
    w = specials((n, k), seed=n + k) if kind == "specials" else gen("heavy_f32", n + k, (n, k))
    amap = random_map((k, n), n + 2 * k)
    pt = packed.pack_transposed(w, amap)
    want = packed.pack(w.T.copy(), amap)
    assert pt.shape == (k, n) and pt.layout == "rows" and (pt.rows, pt.cols) == (k, n) and pt.nbytes == stream_bytes(amap)
    assert np.array_equal(pt.data, want.data) and np.array_equal(pt.offsets, want.offsets) and np.array_equal(pt.map, amap)
    assert np.array_equal(packed.pack_transposed(torch.from_numpy(w.copy()), amap).data, want.data)
    y = packed.unpack_transposed(pt)
    assert y.shape == (n, k) and y.dtype == np.float32 and y.flags["C_CONTIGUOUS"]
    bits = expected_bits(np.ascontiguousarray(w.T), amap).T
    assert np.array_equal(y.view(np.uint32), bits)
    if kind == "heavy":                                  # the budget maps' own transposed reconstruction (no NaN payloads to compare)
        assert np.array_equal(y.view(np.uint32), budget_maps.reconstruct_emulation(w, amap, "transpose").view(np.uint32))
    half = packed.unpack_transposed(pt, dtype="bfloat16")
    assert half.dtype == torch.bfloat16 and tuple(half.shape) == (n, k)
    assert np.array_equal(half.view(torch.int16).numpy().view(np.uint16), (bits >> np.uint32(16)).astype(np.uint16))


@pytest.mark.parametrize("with_bias", [False, True])
def test_emulation_matmul_is_the_float64_product(with_bias):
    n, k = 40, 100
    w = gen("heavy_f32", 5, (n, k))
    amap = random_map((k, n), 6)
    x = to_bf16_valued(gen("normal_f32", 7, (9, k)))
    b = gen("normal_f32", 8, (n,)) if with_bias else None
    pt = packed.pack_transposed(w, amap)
    phat = expected_bits(np.ascontiguousarray(w.T), amap).view(np.float32).astype(np.float64)
    want = x.astype(np.float64) @ phat + (b.astype(np.float64)[None, :] if with_bias else 0.0)
    got = packed.matmul(x, pt, bias=b)
    assert got.shape == (9, n) and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got, packed.matmul(torch.from_numpy(x).to(torch.bfloat16), pt, bias=None if b is None else torch.from_numpy(b)))
    yb = packed.matmul(x, pt, bias=b, out_dtype="bfloat16")
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))
    # an input-major weight packed in the row layout is the same call: x @ W
    wkn = np.ascontiguousarray(w.T)
    assert np.array_equal(packed.matmul(x, packed.pack(wkn, amap), bias=b), got)
    # and the linear layer of the transposed weight in the row layout agrees to the last bit in float64
    ref = packed.pack(np.ascontiguousarray(phat.T.astype(np.float32)), np.zeros((2, 4), dtype=np.int8))
    assert np.array_equal(packed.linear(x, ref, bias=b), got)
    mod = packed.PackedMatmul(pt, bias=b, out_dtype="bfloat16")
    assert mod.backend == "emulation" and (mod.in_features, mod.out_features) == (k, n)
    xt = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(mod(xt.reshape(3, 3, k)).reshape(9, n), yb)
    assert tuple(mod(xt[:0]).shape) == (0, n)


def test_refusals():
    w = gen("heavy_f32", 3, (40, 100))
    amap = random_map((100, 40), 4)
    with pytest.raises(hb.MtqError, match="2-D"):
        packed.pack_transposed(w.reshape(2, 20, 100), amap)
    with pytest.raises(hb.MtqError, match="2-D"):
        packed.pack_transposed(w.reshape(-1), amap)
    with pytest.raises(hb.MtqError, match="transpose's grid"):                   # a map over W's own grid: 2 x 4, not 4 x 2
        packed.pack_transposed(w, random_map((40, 100), 4))
    with pytest.raises(hb.MtqError, match="entries"):
        packed.pack_transposed(w, random_map((100, 72), 4))
    with pytest.raises(hb.MtqError, match="codes"):
        packed.pack_transposed(w, np.full((4, 2), 4, dtype=np.int8))
    with pytest.raises(hb.MtqError, match="backend"):
        packed.pack_transposed(w, amap, backend="cuda")
    pt = packed.pack_transposed(w, amap)
    with pytest.raises(hb.MtqError, match=r"x must be \(m, 100\)"):
        packed.matmul(np.zeros((3, 40), dtype=np.float32), pt)
    with pytest.raises(hb.MtqError, match="out_dtype"):
        packed.matmul(np.zeros((3, 100), dtype=np.float32), pt, out_dtype="float16")
    with pytest.raises(hb.MtqError, match="dtype"):
        packed.unpack_transposed(pt, dtype="float16")
    rank3 = packed.pack(gen("heavy_f32", 5, (2, 32, 64)), random_map((64, 64), 1))
    for call in (lambda: packed.matmul(np.zeros((3, 64), dtype=np.float32), rank3), lambda: packed.unpack_transposed(rank3),
                 lambda: packed.PackedMatmul(rank3)):
        with pytest.raises(hb.MtqError, match="2-D"):
            call()
    # every existing refusal of a transposed map stays, with "row layout" in it; no new layout value exists
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.pack(w, random_map((40, 100), 4), layout="transpose")
    pt.layout = "transpose"
    for call in (lambda: packed.matmul(np.zeros((3, 100), dtype=np.float32), pt), lambda: packed.unpack_transposed(pt),
                 lambda: packed.unpack(pt), lambda: packed.linear(np.zeros((3, 40), dtype=np.float32), pt)):
        with pytest.raises(hb.MtqError, match="row layout"):
            call()


def test_save_and_load_need_nothing_new(tmp_path):
    w = gen("heavy_f32", 9, (72, 300))
    amap = random_map((300, 72), 10)
    pt = packed.pack_transposed(w, amap)
    packed.save(tmp_path / "p.npz", pt)
    back = packed.load(tmp_path / "p.npz")
    assert back.shape == (300, 72) and back.layout == "rows" and np.array_equal(back.data, pt.data)
    assert np.array_equal(packed.unpack_transposed(back).view(np.uint32), packed.unpack_transposed(pt).view(np.uint32))


def _script(name="pack_mixed_tile_assignment"):
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NAME = "model.layers.0.attn.k.weight"


def _weight():
    x = model_source.build_model_index("synthetic:tiny").load(NAME).float().numpy()
    assert x.ndim == 2
    return x


def test_cli_store_transposed_verify_and_unpack(tmp_path, capsys):
    cli = _script()
    w = _weight()
    n, k = w.shape
    amap = random_map((k, n), 9)
    np.save(tmp_path / "a.npy", amap)
    out = tmp_path / "p.npz"
    base = ["pack", "synthetic:tiny", NAME, str(tmp_path / "a.npy"), "--out", str(out)]
    # a transposed map alone is refused as before, with "row layout" in the output
    assert cli.main(base + ["--layout", "transpose"]) == 1
    assert "row layout" in capsys.readouterr().out and not out.exists()
    # the flag without the layout it belongs to is refused too
    assert cli.main(base + ["--store-transposed"]) == 1
    assert "--layout transpose" in capsys.readouterr().out and not out.exists()
    assert cli.main(base + ["--layout", "transpose", "--store-transposed", "--verify"]) == 0
    text = capsys.readouterr().out
    assert f"packed bytes {stream_bytes(amap)} " in text and "verify: ok" in text and f"({k}, {n})" in text
    pt = packed.load(out)
    assert pt.shape == (k, n) and pt.layout == "rows" and np.array_equal(pt.data, packed.pack(w.T.copy(), amap).data)
    # what --verify compared with: the reconstruct script's --layout transpose output, bit for bit
    recon = _script("reconstruct_mixed_tile_assignment")
    assert recon.main(["synthetic:tiny", NAME, str(tmp_path / "a.npy"), "--layout", "transpose", "--out", str(tmp_path / "r.npy")]) == 0
    want = np.load(tmp_path / "r.npy")
    assert cli.main(["unpack", str(out), "--transposed", "--out", str(tmp_path / "y.npy")]) == 0
    y = np.load(tmp_path / "y.npy")
    assert y.shape == (n, k) and np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(y.view(np.uint32), expected_bits(np.ascontiguousarray(w.T), amap).T)
    assert cli.main(["unpack", str(out), "--out", str(tmp_path / "yt.npy")]) == 0                   # without the flag: the stored (k, n) tensor
    assert np.array_equal(np.load(tmp_path / "yt.npy"), y.T)
    # a stream that no longer holds the reconstruction is reported with a non-zero exit
    capsys.readouterr()
    real = packed.unpack_transposed

    def flipped(pt, **kw):
        pt.data = pt.data.copy()
        pt.data[100] ^= 0x10
        return real(pt, **kw)

    cli.packed.unpack_transposed = flipped
    try:
        assert cli.main(base + ["--layout", "transpose", "--store-transposed", "--verify"]) == 2
    finally:
        cli.packed.unpack_transposed = real
    assert "MISMATCH" in capsys.readouterr().out
    # a tensor of another rank cannot be stored transposed
    assert cli.main(["pack", "synthetic:tiny", "model.layers.0.norm.weight", str(tmp_path / "a.npy"), "--out", str(out), "--layout", "transpose",
                     "--store-transposed"]) == 1
    assert "2-D" in capsys.readouterr().out


def test_a_budget_map_saved_for_the_transposed_layout_round_trips(tmp_path, capsys):
    """The map scripts/layer_output_error.py --transpose --budget-bits B --save-maps writes for the weight basis: the allocation over the
    transposed tile-error table, saved as maps/<op>/budget_<B>_weight_transpose.npy over Wᵀ's grid."""
    cli = _script()
    w = _weight()
    n, k = w.shape
    h = np.broadcast_to(np.eye(32), (-(-k // 32), 32, 32)).copy()
    _e_out, e_w = budget_maps.tile_error_tables_emulation(w, h, layout="transpose")
    made = budget_maps.allocate(e_w, hb.MIXED_TILE_FORMATS, 6.0, grid=budget_maps.tiles_hw(k, n))
    assert not isinstance(made, str), made
    amap = made[0]
    assert amap.shape == budget_maps.tiles_hw(k, n) and len(np.unique(amap)) > 1
    d = tmp_path / "maps" / "k_proj"
    d.mkdir(parents=True)
    path = d / f"budget_{budget_maps.bits_tag(6.0)}_weight_transpose.npy"
    np.save(path, amap)
    out = tmp_path / "k_proj.npz"
    assert cli.main(["pack", "synthetic:tiny", NAME, str(path), "--layout", "transpose", "--store-transposed", "--verify", "--out", str(out)]) == 0
    assert "verify: ok" in capsys.readouterr().out
    pt = packed.load(out)
    assert np.array_equal(packed.unpack_transposed(pt).view(np.uint32), budget_maps.reconstruct_emulation(w, amap, "transpose").view(np.uint32))
