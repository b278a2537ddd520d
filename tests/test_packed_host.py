"""CPU-only: the packed mixed-tile format (include/mtq.h, quantization_analysis_amd/packed.py).  The NumPy encoder / decoder round-trips
to the oracle's bits, a hand-worked tile pins the byte layout, the host entry points and the argument checks of the device entry points
work with no device present, the binding's wrappers check what a launch would dereference, and the CLI packs, verifies and unpacks."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import model_source, packed
from tests.inputs import gen
from tests.packed_cases import TILE_BYTES, expected_bits, random_map, specials, stream_bytes, uniform_map

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(32, 32), (96, 160), (70, 50), (100,), ()]
KINDS = ["normal_bf16", "normal_f32", "heavy_bf16", "heavy_f32", "specials"]


def _input(kind, shape):
    return specials(shape) if kind == "specials" else gen(kind, 5, shape)


def _maps(shape):
    shape2d = orc.flatten_2d(np.zeros(shape, dtype=np.float32))[0].shape
    return [uniform_map(shape2d, c) for c in range(4)] + [random_map(shape2d, 17)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_emulation_round_trip_is_the_oracle_bit_for_bit(kind, shape):
    x = _input(kind, shape)
    for amap in _maps(shape):
        pt = packed.pack(x, amap, backend="emulation")
        y = packed.unpack(pt, backend="emulation")
        want = expected_bits(x, amap)
        assert y.shape == want.shape == np.shape(x) and y.dtype == np.float32
        assert np.array_equal(np.asarray(y).view(np.uint32), want), (kind, shape, amap.reshape(-1)[:4])
        half = packed.unpack(pt, backend="emulation", dtype="bfloat16")     # exact: every value has its low 16 bits zero
        assert np.all(want & np.uint32(0xFFFF) == 0)
        assert np.array_equal(half.view(__import__("torch").int16).numpy().view(np.uint16).astype(np.uint32) << np.uint32(16), want)
        again = packed.pack(x, amap, backend="emulation")
        assert np.array_equal(again.data, pt.data) and pt.data.dtype == np.uint8


def _hand_tile():
    x = np.zeros((32, 32), dtype=np.float32)
    x[0, :8] = [1.0, -1.0, 0.5, 0.75, 1.5, -0.75, 0.0, 0.25]       # group 0: shared exponent 127
    x[1, 16] = 2.0                                                  # group 3 (row 1, half 1): shared exponent 128
    return x


def test_hand_worked_tile_pins_the_byte_layout():
    """Group 0 against exponent 127: man = (1.f << 23) >> d, cut to M bits, ties to even, saturated.
      bfp8 (shift 17): 1 → 0x40, −1 → 0xC0, 0.5 → 0x20, 0.75 → 0x30, 1.5 → 0x60, −0.75 → 0xB0, 0 → 0, 0.25 → 0x10
      bfp4 (shift 21): 4, 12, 2, 3, 6, 11, 0, 1
      bfp2 (shift 23): 1, 3, 0 (0.5 is a tie, even stays), 1 (0.75 rounds up), 1 (1.5: tie to 2, saturates at 1), 3, 0, 0"""
    x = _hand_tile()
    exps = np.zeros(64, dtype=np.uint8)
    exps[0], exps[3] = 127, 128
    codes8 = [0x40, 0xC0, 0x20, 0x30, 0x60, 0xB0, 0x00, 0x10]

    pt = packed.pack(x, uniform_map((32, 32), 1))
    assert pt.data.size == 1088 and np.array_equal(pt.data[:64], exps)
    body = pt.data[64:]
    assert list(body[:8]) == codes8 and body[32 * 1 + 16] == 0x40             # one byte per element, e = 32 * row + col
    assert np.count_nonzero(body) == 8

    pt = packed.pack(x, uniform_map((32, 32), 2))
    assert pt.data.size == 576 and np.array_equal(pt.data[:64], exps)
    body = pt.data[64:]
    assert list(body[:4]) == [0xC4, 0x32, 0xB6, 0x10]                          # even e in the low nibble
    assert body[(32 + 16) // 2] == 0x04 and np.count_nonzero(body) == 5

    pt = packed.pack(x, uniform_map((32, 32), 3))
    assert pt.data.size == 320 and np.array_equal(pt.data[:64], exps)
    body = pt.data[64:]
    assert list(body[:2]) == [0x4D, 0x0D]                                      # e at bits 2 * (e % 4): 1 | 3 << 2 | 0 << 4 | 1 << 6, then 1 | 3 << 2
    assert body[(32 + 16) // 4] == 0x01 and np.count_nonzero(body) == 3

    b = np.zeros((32, 32), dtype=np.uint32)
    b[0, 1], b[0, 2], b[0, 3], b[31, 31] = 0x3F800000, 0x3F808000, 0x3F818000, 0xC0490FDB   # 1.0; a tie to even; a tie to odd + 1; −π
    pt = packed.pack(b.view(np.float32), uniform_map((32, 32), 0))
    assert pt.data.size == 2048
    assert list(pt.data[2:8]) == [0x80, 0x3F, 0x80, 0x3F, 0x82, 0x3F]          # little-endian uint16, row-major
    assert list(pt.data[2046:]) == [0x49, 0xC0] and np.count_nonzero(pt.data) == 8


def test_sizes_offsets_and_the_host_entry_points():
    L = hb.lib()
    assert [int(L.mtq_packed_tile_bytes(f)) for f in (-1, 0, 1, 2, 3, 4, 7)] == [0, 2048, 1088, 576, 320, 0, 0]
    assert hb.PACKED_TILE_BYTES == TILE_BYTES and all(b % 64 == 0 for b in TILE_BYTES)
    x = gen("heavy_f32", 2, (96, 160))
    for amap in _maps((96, 160)):
        pt = packed.pack(x, amap)
        counts = np.bincount(amap.reshape(-1), minlength=4)
        assert pt.nbytes == int(np.dot(counts, TILE_BYTES)) == stream_bytes(amap) == pt.data.size
        assert pt.total_bytes == pt.nbytes + amap.size + 4 * (amap.size + 1)
        sizes = np.asarray(TILE_BYTES)[amap.reshape(-1)]
        want = np.concatenate([[0], np.cumsum(sizes)]) // 64
        assert pt.offsets.dtype == np.uint32 and np.array_equal(pt.offsets, want) and int(pt.offsets[-1]) * 64 == pt.nbytes
        assert np.array_equal(hb.packed_offsets(amap), pt.offsets)
        assert pt.counts() == {f: int(c) for f, c in zip(hb.MIXED_TILE_FORMATS, counts)}
    # the real bytes per element beside the size model's constants
    assert [b / 1024 for b in TILE_BYTES] == [2.0, 1.0625, 0.5625, 0.3125]


def test_save_load_round_trip_and_version_check(tmp_path):
    for shape in ((70, 50), (100,), (), (3, 40, 64)):
        x = specials(shape)
        amap = random_map(orc.flatten_2d(x)[0].shape, 4)
        pt = packed.pack(x, amap)
        packed.save(tmp_path / "p.npz", pt)
        back = packed.load(tmp_path / "p.npz")
        assert back.shape == tuple(shape) and back.shape_info[0] == pt.shape_info[0] and (back.rows, back.cols) == (pt.rows, pt.cols)
        assert np.array_equal(back.map, pt.map) and np.array_equal(back.offsets, pt.offsets) and np.array_equal(back.data, pt.data)
        assert np.array_equal(np.asarray(packed.unpack(back)).view(np.uint32), expected_bits(x, amap))
    with np.load(tmp_path / "p.npz") as z:
        fields = {k: z[k] for k in z.files}
    assert int(fields["format_version"]) == packed.FORMAT_VERSION
    np.savez(tmp_path / "new.npz", **{**fields, "format_version": np.int64(packed.FORMAT_VERSION + 1)})
    with pytest.raises(hb.MtqError, match="version"):
        packed.load(tmp_path / "new.npz")
    np.savez(tmp_path / "none.npz", **{k: v for k, v in fields.items() if k != "format_version"})
    with pytest.raises(hb.MtqError, match="version"):
        packed.load(tmp_path / "none.npz")
    np.savez(tmp_path / "short.npz", **{**fields, "data": fields["data"][:-64]})
    with pytest.raises(hb.MtqError, match="stream"):
        packed.load(tmp_path / "short.npz")


def test_transposed_maps_and_bad_codes_are_refused():
    x = gen("normal_f32", 1, (64, 64))
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.pack(x, uniform_map((64, 64), 1), layout="transpose")
    bad = uniform_map((64, 64), 1)
    bad[1, 1] = 4
    with pytest.raises(hb.MtqError, match="codes"):
        packed.pack(x, bad)
    with pytest.raises(hb.MtqError, match="entries"):
        packed.pack(x, uniform_map((64, 96), 1))
    pt = packed.pack(x, uniform_map((64, 64), 1))
    pt.layout = "transpose"
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.unpack(pt)


def test_emulation_linear_is_the_float64_product():
    w = gen("heavy_bf16", 3, (70, 100))
    amap = random_map((70, 100), 6)
    pt = packed.pack(w, amap)
    x = gen("normal_bf16", 4, (5, 100)) * 50
    b = gen("normal_f32", 5, (70,))
    what = expected_bits(w, amap).view(np.float32).astype(np.float64)
    want = (x.astype(np.float64) @ what.T + b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(packed.linear(x, pt, bias=b), want)
    with pytest.raises(hb.MtqError, match=r"\(m, 100\)"):
        packed.linear(x[:, :64], pt)


def test_c_abi_argument_errors_need_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    amap = np.array([0, 1, 2, 9], dtype=np.int8)
    off = np.zeros(5, dtype=np.uint32)
    assert L.mtq_packed_offsets(amap.ctypes.data, 4, off.ctypes.data) == -1 and b"map[3]" in L.mtq_last_error()
    assert L.mtq_packed_offsets(None, 4, off.ctypes.data) == -1 and L.mtq_packed_offsets(amap.ctypes.data, 4, None) == -1
    assert L.mtq_packed_offsets(amap.ctypes.data, 0, off.ctypes.data) == -1
    assert L.mtq_packed_offsets(amap.ctypes.data, 3, off.ctypes.data) == 0 and list(off[:4]) == [0, 32, 49, 58]

    big = 1 << 20
    # pack: x, in_dtype, rows, cols, ld, map, offsets, out, out_bytes, stream
    ok = (p, 0, 64, 64, 64, p, p, p, big, None)

    def pack(**kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_pack_tiles(*args)

    for null in (0, 5, 6, 7):
        assert pack(**{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert pack(a1=7) == -1 and b"in_dtype" in L.mtq_last_error()
    assert pack(a4=63) == -1 and b"ld < cols" in L.mtq_last_error()
    assert pack(a2=0) == -1 and pack(a3=-1) == -1
    assert pack(a8=4 * 320 - 1) == -1 and b"smaller than the stream" in L.mtq_last_error()
    assert pack(a7=p + 8) == -1 and b"aligned" in L.mtq_last_error()

    # unpack: packed, packed_bytes, map, offsets, rows, cols, y, out_dtype, ldy, stream
    oku = (p, big, p, p, 64, 64, p, 1, 64, None)

    def unpack(**kw):
        args = list(oku)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_unpack_tiles(*args)

    for null in (0, 2, 3, 6):
        assert unpack(**{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert unpack(a7=2) == -1 and b"out_dtype" in L.mtq_last_error()
    assert unpack(a8=63) == -1 and b"ldy < cols" in L.mtq_last_error()
    assert unpack(a1=4 * 320 - 1) == -1 and b"smaller than the stream" in L.mtq_last_error()
    assert unpack(a0=p + 4) == -1 and b"aligned" in L.mtq_last_error()

    # linear: x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream
    okl = (p, 3, 64, 64, p, big, p, p, 64, None, p, 1, 64, None)

    def linear(**kw):
        args = list(okl)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_packed_linear(*args)

    for null in (0, 4, 6, 7, 10):
        assert linear(**{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert linear(a11=5) == -1 and b"out_dtype" in L.mtq_last_error()
    assert linear(a3=63) == -1 and b"ldx < k" in L.mtq_last_error()
    assert linear(a12=63) == -1 and b"ldy < n" in L.mtq_last_error()
    assert linear(a1=0) == -1 and linear(a2=0) == -1 and linear(a8=0) == -1
    assert linear(a5=4 * 320 - 1) == -1 and b"smaller than the stream" in L.mtq_last_error()
    import torch

    if not torch.cuda.is_available():     # everything in order: only the device is missing
        assert pack() == -3 and unpack() == -3 and linear() == -3


class _OnDevice:
    """A host tensor that passes for a device tensor in the binding's checks, with a null pointer (test_capi_host.py): a call that got
    past every check is refused by the library's own null check, never launched."""

    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return 0


def test_wrappers_check_what_they_dereference():
    import torch

    def D(*shape, dtype=torch.uint8):
        return _OnDevice(torch.zeros(shape, dtype=dtype))

    amap = random_map((64, 96), 3)
    T = amap.size
    nbytes = stream_bytes(amap)
    with pytest.raises(hb.MtqError, match="codes"):
        hb.PackedTables(np.full((2, 3), 4, dtype=np.int8), D(T, dtype=torch.int8), D(T + 1, dtype=torch.int32))
    with pytest.raises(hb.MtqError, match="2-D"):
        hb.PackedTables(amap.reshape(-1), D(T, dtype=torch.int8), D(T + 1, dtype=torch.int32))
    with pytest.raises(hb.MtqError, match="device map"):
        hb.PackedTables(amap, D(T - 1, dtype=torch.int8), D(T + 1, dtype=torch.int32))
    with pytest.raises(hb.MtqError, match="device map"):
        hb.PackedTables(amap, torch.zeros(T, dtype=torch.int8), D(T + 1, dtype=torch.int32))          # host memory
    with pytest.raises(hb.MtqError, match="device offsets"):
        hb.PackedTables(amap, D(T, dtype=torch.int8), D(T, dtype=torch.int32))
    with pytest.raises(hb.MtqError, match="device offsets"):
        hb.PackedTables(amap, D(T, dtype=torch.int8), D(T + 1, dtype=torch.int64))
    tables = hb.PackedTables(amap, D(T, dtype=torch.int8), D(T + 1, dtype=torch.int32))
    assert tables.nbytes == nbytes and (tables.tiles_h, tables.tiles_w) == (2, 3)

    x = torch.zeros((64, 96), dtype=torch.bfloat16)
    for bad, msg in ((x, "device tensor"), (_OnDevice(x[None]), "2-D"), (_OnDevice(torch.zeros((64, 192))[:, ::2]), "contiguous rows"),
                     (_OnDevice(x.half()), "bfloat16 or float32"), (_OnDevice(x[:, :64]), "tiles")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles(bad, tables, out=D(nbytes))
    for out, msg in ((D(nbytes - 1), "out"), (torch.zeros(nbytes, dtype=torch.uint8), "out"), (D(nbytes, dtype=torch.int8), "out")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles(_OnDevice(x), tables, out=out)
    with pytest.raises(hb.MtqError, match="null argument"):                    # every check passed (a larger buffer too): the library's turn
        hb.pack_tiles(_OnDevice(x), tables, out=D(nbytes + 64), stream=None)

    y = D(64, 96, dtype=torch.float32)
    with pytest.raises(hb.MtqError, match="data"):
        hb.unpack_tiles(D(nbytes - 64), tables, 64, 96, out=y)
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.unpack_tiles(D(nbytes), tables, 64, 97, out=y)
    with pytest.raises(hb.MtqError, match="output type"):
        hb.unpack_tiles(D(nbytes), tables, 64, 96, dtype=torch.float16, out=y)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.unpack_tiles(D(nbytes), tables, 64, 96, dtype=torch.bfloat16, out=y)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.unpack_tiles(D(nbytes), tables, 64, 96, out=torch.zeros((64, 96)))
    with pytest.raises(hb.MtqError, match="null argument"):
        hb.unpack_tiles(D(nbytes), tables, 64, 96, out=y, stream=None)

    xa = _OnDevice(torch.zeros((5, 96), dtype=torch.bfloat16))
    yo = D(5, 64, dtype=torch.float32)
    with pytest.raises(hb.MtqError, match="bfloat16"):
        hb.packed_linear(_OnDevice(torch.zeros((5, 96))), D(nbytes), tables, 64, out=yo)
    with pytest.raises(hb.MtqError, match="tiles"):
        hb.packed_linear(_OnDevice(torch.zeros((5, 128), dtype=torch.bfloat16)), D(nbytes), tables, 64, out=yo)
    with pytest.raises(hb.MtqError, match="data"):
        hb.packed_linear(xa, D(nbytes - 1), tables, 64, out=yo)
    with pytest.raises(hb.MtqError, match="bias"):
        hb.packed_linear(xa, D(nbytes), tables, 64, bias=D(63, dtype=torch.float32), out=yo)
    with pytest.raises(hb.MtqError, match="bias"):
        hb.packed_linear(xa, D(nbytes), tables, 64, bias=torch.zeros(64), out=yo)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.packed_linear(xa, D(nbytes), tables, 64, out=D(5, 63, dtype=torch.float32))
    with pytest.raises(hb.MtqError, match="null argument"):
        hb.packed_linear(xa, D(nbytes), tables, 64, bias=D(64, dtype=torch.float32), out=yo, stream=None)


def test_header_comments_name_only_declared_functions():
    """test_capi_host.py reads every `mtq_name(` of the header as a declaration: the packed section keeps to that."""
    hdr = (ROOT / "include" / "mtq.h").read_text()
    for name in ("mtq_packed_tile_bytes", "mtq_packed_offsets", "mtq_pack_tiles", "mtq_unpack_tiles", "mtq_packed_linear"):
        assert len(re.findall(rf"\b{name}\s*\(", hdr)) == 1 and hb.SIGNATURES[name][2] is True
    assert hb.lib().mtq_version() == 143


def _script():
    import importlib.util

    spec = importlib.util.spec_from_file_location("pack_mixed_tile_assignment", ROOT / "scripts" / "pack_mixed_tile_assignment.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_pack_verify_and_unpack(tmp_path, capsys):
    cli = _script()
    idx = model_source.build_model_index("synthetic:tiny")
    for name in ("model.layers.0.attn.k.weight", "model.layers.0.norm.weight", "model.layers.0.attn.q.weight"):
        x = idx.load(name).float().numpy()
        amap = random_map(orc.flatten_2d(x)[0].shape, 9)
        np.save(tmp_path / "a.npy", amap)
        out = tmp_path / "p.npz"
        assert cli.main(["pack", "synthetic:tiny", name, str(tmp_path / "a.npy"), "--out", str(out), "--backend", "emulation", "--verify"]) == 0
        text = capsys.readouterr().out
        assert f"packed bytes {stream_bytes(amap)} " in text and "size-model bytes" in text and "verify: ok" in text
        assert cli.main(["unpack", str(out), "--out", str(tmp_path / "y.npy")]) == 0
        y = np.load(tmp_path / "y.npy")
        assert np.array_equal(y.view(np.uint32), expected_bits(x, amap))
    # a name mapping, as reconstruct_mixed_tile_assignment.py takes it
    (tmp_path / "m.json").write_text('{"int_to_format": ["bfp2", "bfp4", "bfp8", "bf16"]}')
    assert cli.main(["pack", "synthetic:tiny", name, str(tmp_path / "a.npy"), "--assignment-mapping", str(tmp_path / "m.json"), "--out", str(out), "--verify"]) == 0
    assert np.array_equal(packed.load(out).map, 3 - amap)
    capsys.readouterr()
    assert cli.main(["pack", "synthetic:tiny", name, str(tmp_path / "a.npy"), "--out", str(out), "--layout", "transpose"]) == 1
    assert "row layout" in capsys.readouterr().out
    # a stream that no longer holds the reconstruction is reported with a non-zero exit
    real = packed.unpack

    def flipped(pt, **kw):
        pt.data = pt.data.copy()
        pt.data[100] ^= 0x10
        return real(pt, **kw)

    cli.packed.unpack = flipped
    try:
        assert cli.main(["pack", "synthetic:tiny", name, str(tmp_path / "a.npy"), "--out", str(out), "--verify"]) == 2
    finally:
        cli.packed.unpack = real
    assert "MISMATCH" in capsys.readouterr().out
