"""CPU-only: batches of packed weights in the transposed layout (packed.pack_batch_transposed / unpack_batch_transposed on the emulation
backend), scripts/pack_model.py --store-transposed on the emulation backend with packed.read_index, and the argument checks of the two
batched transposed C entry points, which need no device.

Every shape has n != k, so an entry that swapped an axis could not pass."""
import functools
import json

import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import model_source, packed
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.tile_search import TileStats, reconstruct
from tests.inputs import gen
from tests.packed_cases import expected_bits, random_map, specials
from tests.test_packed_batch_host import GREEDY, TRANSPOSED, pack_model_script

# (name, count, n, k): W is (n, k), its packed transpose (k, n)
SHAPES = [("3x70x100", 3, 70, 100), ("4x64x96", 4, 64, 96), ("2x33x31", 2, 33, 31), ("2x1x40", 2, 1, 40), ("2x40x1", 2, 40, 1)]


def transposed_maps(count, n, k, seed):
    """Random maps over the grid of the (k, n) transposes, every code present where the grid has room for it."""
    maps = np.stack([random_map((k, n), seed + i) for i in range(count)])
    flat = maps.reshape(count, -1)
    if flat.shape[1] >= 4:
        flat[0, :4] = [0, 1, 2, 3]
    else:
        flat[:, 0] = np.arange(count) % 4
    return maps


@functools.lru_cache(maxsize=None)
def batch(name):
    """(float32 (count, n, k), maps (count, ceil(k/32), ceil(n/32))) — computed once, shared, never written to."""
    _n, count, n, k = next(s for s in SHAPES if s[0] == name)
    if name == "3x70x100":
        w = np.stack([specials((n, k), seed=11 + i) for i in range(count)])
    else:
        w = np.stack([gen("heavy_f32", 60 + i, (n, k)) for i in range(count)])
    maps = transposed_maps(count, n, k, 50)
    w.setflags(write=False)
    maps.setflags(write=False)
    return w, maps


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_batch_is_pack_transposed_per_tensor_back_to_back(name):
    w, maps = batch(name)
    count, n, k = w.shape
    pts = packed.pack_batch_transposed(w, maps)
    singles = [packed.pack_transposed(w[i], maps[i]) for i in range(count)]
    b = packed.batch_of(pts)
    assert b is not None and (b.count, b.rows, b.cols) == (count, k, n) and len(pts) == count
    for pt, one in zip(pts, singles):
        assert pt.shape == one.shape == (k, n) and (pt.rows, pt.cols) == (k, n) and pt.layout == "rows"
        assert np.array_equal(pt.data, one.data) and np.array_equal(pt.offsets, one.offsets) and np.array_equal(pt.map, one.map)
        assert np.shares_memory(pt.data, b.arena)
    assert b.arena.dtype == np.uint8 and np.array_equal(b.arena, np.concatenate([one.data for one in singles]))
    assert np.array_equal(b.bases.astype(np.int64) * 64, np.concatenate([[0], np.cumsum([one.nbytes for one in singles])]))


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_round_trip_gives_w_back_in_its_own_orientation(name):
    import torch

    w, maps = batch(name)
    count, n, k = w.shape
    pts = packed.pack_batch_transposed(w, maps)
    y = packed.unpack_batch_transposed(pts)
    assert y.shape == (count, n, k) and y.dtype == np.float32 and y.flags["C_CONTIGUOUS"]
    yt = packed.unpack_batch(pts)                                                   # the same list, unpacked as what it is: the transposes
    assert yt.shape == (count, k, n)
    for i in range(count):
        want = np.ascontiguousarray(expected_bits(np.ascontiguousarray(w[i].T), maps[i]).T)
        assert np.array_equal(y[i].view(np.uint32), want), (name, i)
        assert np.array_equal(np.asarray(packed.unpack_transposed(pts[i])).view(np.uint32), want), (name, i)
        assert np.array_equal(yt[i].view(np.uint32), want.T), (name, i)
    half = packed.unpack_batch_transposed(pts, dtype="bfloat16")
    assert half.dtype == torch.bfloat16 and tuple(half.shape) == (count, n, k)
    assert np.array_equal(half.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << np.uint32(16), y.view(np.uint32))
    # any list of one shape, tensor by tensor
    assert np.array_equal(packed.unpack_batch_transposed(pts[::-1]).view(np.uint32), y[::-1].view(np.uint32))


def test_products_are_ordinary_packed_tensors(tmp_path):
    w, maps = batch("4x64x96")
    pts = packed.pack_batch_transposed(w, maps)
    assert packed.as_batch(pts) is packed.batch_of(pts)
    x = gen("normal_f32", 9, (5, 96))
    alone = packed.pack_transposed(w[2], maps[2])
    assert np.array_equal(packed.matmul(x, pts[2]).view(np.uint32), packed.matmul(x, alone).view(np.uint32))
    packed.save_dir(tmp_path / "d", {f"w{i}": pt for i, pt in enumerate(pts)}, meta={"w0": {"stored": "transpose", "source_shape": [64, 96]}})
    back = packed.load_dir(tmp_path / "d")
    assert all(np.array_equal(back[f"w{i}"].data, pts[i].data) and back[f"w{i}"].shape == (96, 64) for i in range(4))
    index = packed.read_index(tmp_path / "d")
    assert index == json.loads((tmp_path / "d" / "index.json").read_text()) and index["tensors"]["w0"]["stored"] == "transpose"
    assert "stored" not in index["tensors"]["w1"] and index["tensors"]["w0"]["shape"] == [96, 64]


def test_read_index_refuses_what_load_dir_refuses(tmp_path):
    with pytest.raises(hb.MtqError, match="index.json is missing"):
        packed.read_index(tmp_path)
    (tmp_path / "index.json").write_text(json.dumps({"format_version": packed.FORMAT_VERSION + 1, "tensors": {}}))
    with pytest.raises(hb.MtqError, match="format version"):
        packed.read_index(tmp_path)
    (tmp_path / "index.json").write_text("[]")
    with pytest.raises(hb.MtqError, match="format version"):
        packed.read_index(tmp_path)


def test_refusals():
    w, maps = batch("3x70x100")
    assert maps.shape == (3, 4, 3)
    with pytest.raises(hb.MtqError, match="transposes' grid"):
        packed.pack_batch_transposed(w, np.ascontiguousarray(maps.transpose(0, 2, 1)))      # the untransposed grid, 3x3x4
    with pytest.raises(hb.MtqError, match="transposes' grid"):
        packed.pack_batch_transposed(w, maps[:2])
    for code in (4, -1):
        bad = maps.copy()
        bad[1, 2, 1] = code
        with pytest.raises(hb.MtqError, match="tensor 1 .*codes"):
            packed.pack_batch_transposed(w, bad)
    with pytest.raises(hb.MtqError, match="entries"):
        packed.pack_batch_transposed(w, maps.reshape(-1)[:-1])
    with pytest.raises(hb.MtqError, match=r"\(count, n, k\)"):
        packed.pack_batch_transposed(w[0], maps)
    with pytest.raises(hb.MtqError, match=r"\(count, n, k\)"):
        packed.pack_batch_transposed(w[:0], maps[:0])
    with pytest.raises(hb.MtqError, match="backend"):
        packed.pack_batch_transposed(w, maps, backend="ttnn")
    with pytest.raises(hb.MtqError, match="row layout"):                             # the row entry keeps refusing: the new name is the entry
        packed.pack_batch(w, maps, layout="transpose")
    pts = packed.pack_batch_transposed(w, maps)
    with pytest.raises(hb.MtqError, match="at least one"):
        packed.unpack_batch_transposed([])
    with pytest.raises(hb.MtqError, match="backend"):
        packed.unpack_batch_transposed(pts, backend="ttnn")
    with pytest.raises(hb.MtqError, match="dtype"):
        packed.unpack_batch_transposed(pts, dtype="float16")
    with pytest.raises(hb.MtqError, match="one 2-D shape"):
        packed.unpack_batch_transposed(pts + packed.pack_batch_transposed(*batch("4x64x96")))
    with pytest.raises(hb.MtqError, match="2-D packed"):
        packed.unpack_batch_transposed([packed.pack(np.zeros((2, 32, 32), dtype=np.float32), np.zeros((2, 1), dtype=np.int8))])
    assert np.array_equal(packed.pack_batch_transposed(w, maps.reshape(3, -1))[1].data, pts[1].data)      # flat maps of the right size are taken


# ----------------------------------------------------------------------------- scripts/pack_model.py --store-transposed

def test_pack_model_store_transposed_on_the_emulation_backend(tmp_path, capsys):
    script = pack_model_script()
    out = tmp_path / "packed"
    argv = ["synthetic:tiny", "--compression-config", str(TRANSPOSED), "--out-dir", str(out), "--backend", "emulation", "--verify", "--store-transposed"]
    assert script.main(argv) == 0
    text = capsys.readouterr().out
    assert "verify: ok (5 tensors" in text and "MISMATCH" not in text
    index = packed.read_index(out)
    run = index["run"]
    assert run["params"]["layout"] == "transpose" and run["layout"] == "transpose" and run["stored"] == "transpose"
    idx = model_source.build_model_index("synthetic:tiny")
    names = model_source.resolve_selected_tensors(idx, None)
    back = packed.load_dir(out)
    assert list(back) == names == list(index["tensors"]) and len(names) == 5
    ranks = set()
    for name in names:
        x = np.asarray(idx.load(name).float().numpy(), dtype=np.float32)
        e, pt = index["tensors"][name], back[name]
        ranks.add(x.ndim)
        assert e["stored"] == "transpose" and e["source_shape"] == list(x.shape) and e["route"] == "per-tensor" and e["verified"] is True
        assert e["shape"] == list(pt.shape) == list(x.shape[::-1]) and pt.layout == "rows"
        # what reconstruct_mixed_tile_assignment.py --layout transpose gives for the tensor and the stored map: reconstruct() on np.transpose(x)
        x2d, info = packed.flatten_2d(np.transpose(x))
        th, tw = -(-x2d.shape[0] // 32), -(-x2d.shape[1] // 32)
        assert pt.map.shape == (th, tw)
        ts = TileStats(0, th, tw, int(x.size), info, x2d, "emulation", True)
        want = np.ascontiguousarray(np.transpose(np.asarray(reconstruct(ts, pt.map, Quantizer("emulation")), dtype=np.float32)))
        got = np.asarray(packed.unpack_transposed(pt) if x.ndim == 2 else np.transpose(packed.unpack(pt)), dtype=np.float32)
        assert got.shape == x.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32)), name
    assert ranks == {1, 2}                                                           # the vector is its own transpose: pack(x, map)


def test_pack_model_store_transposed_needs_a_transposed_config(tmp_path, capsys):
    script = pack_model_script()
    assert script.main(["synthetic:tiny", "--compression-config", str(GREEDY), "--out-dir", str(tmp_path / "g"), "--store-transposed"]) == 1
    text = capsys.readouterr().out
    assert "--store-transposed" in text and '"layout": "transpose"' in text and not (tmp_path / "g").exists()
    # and without the flag a transposed config is refused as before
    assert script.main(["synthetic:tiny", "--compression-config", str(TRANSPOSED), "--out-dir", str(tmp_path / "t")]) == 1
    assert "row layout" in capsys.readouterr().out and not (tmp_path / "t").exists()


# ----------------------------------------------------------------------------- the C entry points

def test_c_abi_argument_errors_need_no_device():
    L = hb.lib()
    assert hb.PACKED_BATCH_TRANSPOSED == ("mtq_pack_tiles_transposed_batched", "mtq_unpack_tiles_transposed_batched")
    for name in hb.PACKED_BATCH_TRANSPOSED:
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS and name in hb.EXPORTS and getattr(L, name, None) is not None
    assert hb.has_packed_batch_transposed()
    assert hb.SIGNATURES["mtq_pack_tiles_transposed_batched"][:2] == hb.SIGNATURES["mtq_pack_tiles_batched"][:2]
    assert hb.SIGNATURES["mtq_unpack_tiles_transposed_batched"][:2] == hb.SIGNATURES["mtq_unpack_tiles_batched"][:2]
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    rows, cols, tiles = 64, 96, 6                            # the transposes' grid is 3 x 2

    def call(fn, ok, **kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return fn(*args)

    # pack: w, in_dtype, count, rows, cols, ld, stride, maps, offsets, bases, out, out_bytes, stream
    pack = L.mtq_pack_tiles_transposed_batched
    okp = (p, 0, 3, rows, cols, cols, rows * cols, p, p, p, p, big, None)
    for null in (0, 7, 8, 9, 10):
        assert call(pack, okp, **{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert call(pack, okp, a1=7) == -1 and b"in_dtype" in L.mtq_last_error()
    for count in (0, -2):
        assert call(pack, okp, a2=count) == -1 and b"count" in L.mtq_last_error()
    assert call(pack, okp, a3=0) == -1 and call(pack, okp, a4=-1) == -1
    assert call(pack, okp, a5=cols - 1) == -1 and b"ld < cols" in L.mtq_last_error()
    assert call(pack, okp, a6=(rows - 1) * cols + cols - 1) == -1 and b"stride" in L.mtq_last_error()
    assert call(pack, okp, a11=3 * tiles * 320 - 1) == -1 and b"smaller than the streams" in L.mtq_last_error()
    assert call(pack, okp, a10=p + 8) == -1 and b"aligned" in L.mtq_last_error()

    # unpack: packed, packed_bytes, maps, offsets, bases, count, rows, cols, y, out_dtype, ldy, stride, stream
    unpack = L.mtq_unpack_tiles_transposed_batched
    oku = (p, big, p, p, p, 3, rows, cols, p, 1, cols, rows * cols, None)
    for null in (0, 2, 3, 4, 8):
        assert call(unpack, oku, **{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert call(unpack, oku, a9=2) == -1 and b"out_dtype" in L.mtq_last_error()
    for count in (0, -2):
        assert call(unpack, oku, a5=count) == -1 and b"count" in L.mtq_last_error()
    assert call(unpack, oku, a6=0) == -1 and call(unpack, oku, a7=-1) == -1
    assert call(unpack, oku, a10=cols - 1) == -1 and b"ldy < cols" in L.mtq_last_error()
    assert call(unpack, oku, a11=(rows - 1) * cols + cols - 1) == -1 and b"stride" in L.mtq_last_error()
    assert call(unpack, oku, a1=3 * tiles * 320 - 1) == -1 and b"smaller than the streams" in L.mtq_last_error()
    assert call(unpack, oku, a0=p + 4) == -1 and b"aligned" in L.mtq_last_error()
    import torch

    if not torch.cuda.is_available():     # everything in order: only the device is missing, and it is looked for last
        assert call(pack, okp) == -3 and call(unpack, oku) == -3
        assert call(pack, okp, a2=1, a6=0) == -3 and call(unpack, oku, a5=1, a11=0) == -3      # a batch of one: its stride means nothing


class _OnDevice:
    """A host tensor that passes for a device tensor in the binding's checks, with a null pointer (tests/test_packed_batch_host.py): a
    call that got past every check is refused by the library's own null check, never launched."""

    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return 0


def test_wrappers_check_the_transposes_grid_before_the_library():
    import torch

    def D(*shape, dtype=torch.uint8):
        return _OnDevice(torch.zeros(shape, dtype=dtype))

    count, rows, cols = 3, 40, 100                           # W's grid is 2 x 4, the transposes' 4 x 2: 8 tiles either way
    w = _OnDevice(torch.zeros((count, rows, cols), dtype=torch.bfloat16))
    maps, offs, bases = D(count, 8, dtype=torch.int8), D(count, 9, dtype=torch.int32), D(count + 1, dtype=torch.int64)
    arena = D(count * 8 * 2048)
    narrow = _OnDevice(torch.zeros((count, 33, 100), dtype=torch.bfloat16))       # another shape with 8 tiles
    tall = _OnDevice(torch.zeros((count, 100, 65), dtype=torch.bfloat16))         # 12 tiles: not these tables'
    with pytest.raises(hb.MtqError, match="device maps"):
        hb.pack_tiles_transposed_batched(tall, maps, offs, bases, arena)
    for bad, msg in ((torch.zeros((count, rows, cols)), "device tensor"), (_OnDevice(torch.zeros((rows, cols))), "3-D"),
                     (_OnDevice(torch.zeros((count, rows, 2 * cols))[:, :, ::2]), "contiguous rows")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles_transposed_batched(bad, maps, offs, bases, arena)
    with pytest.raises(hb.MtqError, match="out"):
        hb.pack_tiles_transposed_batched(w, maps, offs, bases, D(count * 8 * 320 - 1))
    for ok in (w, narrow):
        with pytest.raises(hb.MtqError, match="null argument"):                     # every check passed: the library's turn
            hb.pack_tiles_transposed_batched(ok, maps, offs, bases, arena, stream=None)
    y = D(count, rows, cols, dtype=torch.float32)
    with pytest.raises(hb.MtqError, match="device offsets"):
        hb.unpack_tiles_transposed_batched(arena, maps, D(count, 8, dtype=torch.int32), bases, count, rows, cols, out=y)
    with pytest.raises(hb.MtqError, match="output type"):
        hb.unpack_tiles_transposed_batched(arena, maps, offs, bases, count, rows, cols, dtype=torch.float16, out=y)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.unpack_tiles_transposed_batched(arena, maps, offs, bases, count, rows, cols, out=D(count, cols, rows, dtype=torch.float32))
    with pytest.raises(hb.MtqError, match="null argument"):
        hb.unpack_tiles_transposed_batched(arena, maps, offs, bases, count, rows, cols, out=y, stream=None)
