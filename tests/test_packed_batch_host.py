"""CPU-only: batches of packed mixed-tile weights (packed.pack_batch / unpack_batch on the emulation backend), directories of packed
tensors (save_dir / load_dir), scripts/pack_model.py on the emulation backend, and the argument checks of the three batched C entry
points, which need no device."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from quantization_analysis_amd import cli, model_source, packed
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms import create_algorithm
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from tests.inputs import gen
from tests.packed_cases import expected_bits, random_map, specials, uniform_map

ROOT = Path(__file__).resolve().parent.parent
GREEDY = ROOT / "compression_configs" / "compression_config.mixed_tile_greedy.example.json"
TRANSPOSED = ROOT / "compression_configs" / "compression_config.mixed_tile_greedy_transpose.example.json"


def _batch(kind, count, shape):
    if kind == "specials":
        x = np.stack([specials(shape, seed=11 + i) for i in range(count)])
    else:
        x = np.stack([gen(kind, 3 + i, shape) for i in range(count)])
    maps = np.stack([random_map(shape, 20 + i) for i in range(count)])
    maps[0].reshape(-1)[:4] = [0, 1, 2, 3]                 # every code present
    return x, maps


@pytest.mark.parametrize("kind,count,shape", [("specials", 3, (70, 100)), ("normal_bf16", 4, (64, 96))], ids=["3x70x100", "4x64x96"])
def test_emulation_batch_is_the_single_packs_back_to_back(kind, count, shape):
    x, maps = _batch(kind, count, shape)
    pts = packed.pack_batch(x, maps, backend="emulation")
    singles = [packed.pack(x[i], maps[i]) for i in range(count)]
    batch = packed.batch_of(pts)
    assert batch is not None and batch.count == count and (batch.rows, batch.cols) == shape
    assert len(pts) == count
    for pt, one in zip(pts, singles):
        assert np.array_equal(pt.data, one.data) and np.array_equal(pt.offsets, one.offsets) and pt.offsets.dtype == np.uint32
        assert np.array_equal(pt.map, one.map) and pt.shape == one.shape == shape and pt.nbytes == one.nbytes == pt.data.size
    assert np.array_equal(batch.arena, np.concatenate([one.data for one in singles])) and batch.arena.dtype == np.uint8
    cum = np.concatenate([[0], np.cumsum([one.nbytes for one in singles])])
    assert batch.bases.dtype == np.uint64 and np.array_equal(batch.bases.astype(np.int64) * 64, cum)
    for i, pt in enumerate(pts):                           # the slices start at 64 * cumsum, inside the one arena
        assert np.shares_memory(pt.data, batch.arena)
        assert pt.data.__array_interface__["data"][0] - batch.arena.__array_interface__["data"][0] == cum[i]
    y = packed.unpack_batch(pts, backend="emulation")
    assert y.shape == (count, *shape) and y.dtype == np.float32
    for i in range(count):
        want = expected_bits(x[i], maps[i])
        assert np.array_equal(y[i].view(np.uint32), want)
        assert np.array_equal(np.asarray(packed.unpack(pts[i])).view(np.uint32), want)      # each one a full citizen
    half = packed.unpack_batch(pts, backend="emulation", dtype="bfloat16")
    import torch

    assert np.array_equal(half.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << np.uint32(16), y.view(np.uint32))
    assert packed.batch_of(pts[:-1]) is None and packed.batch_of(pts[::-1]) is None and packed.batch_of(singles) is None
    assert np.array_equal(packed.unpack_batch(pts[::-1]).view(np.uint32), y[::-1].view(np.uint32))      # any list of one shape, tensor by tensor


def test_pack_batch_refuses_what_pack_refuses():
    x, maps = _batch("normal_f32", 2, (64, 96))
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.pack_batch(x, maps, layout="transpose")
    bad = maps.copy()
    bad[1, 1, 2] = 4
    with pytest.raises(hb.MtqError, match="tensor 1 .*codes"):
        packed.pack_batch(x, bad)
    bad[1, 1, 2] = -1
    with pytest.raises(hb.MtqError, match="tensor 1 .*codes"):
        packed.pack_batch(x, bad)
    with pytest.raises(hb.MtqError, match="entries"):
        packed.pack_batch(x, maps[:1])
    with pytest.raises(hb.MtqError, match="count, rows, cols"):
        packed.pack_batch(x[0], maps)
    with pytest.raises(hb.MtqError, match="backend"):
        packed.pack_batch(x, maps, backend="ttnn")
    with pytest.raises(hb.MtqError, match="shapes"):
        packed.pack_batch(x, maps, shapes=[(64, 96), (96, 64)])
    pts = packed.pack_batch(x, maps, shapes=[(2, 32, 96), (64, 96)])
    assert pts[0].shape == (2, 32, 96) and packed.unpack(pts[0]).shape == (2, 32, 96)
    pts[0].layout = "transpose"
    with pytest.raises(hb.MtqError, match="row layout"):
        packed.unpack_batch(pts)


NAMES = ["model.layers.0.attn.q.weight", "blocks/0/mlp.up:weight", "blocks/0/mlp.up_weight", "norm"]


def _named():
    named = {}
    for i, (name, shape) in enumerate(zip(NAMES, [(70, 50), (64, 96), (64, 96), (100,)])):
        x = specials(shape, seed=30 + i)
        x2 = packed.flatten_2d(x)[0]
        named[name] = (x, packed.pack(x, random_map(x2.shape, 40 + i)))
    return named


def test_save_dir_load_dir_round_trip_keeps_the_names(tmp_path):
    named = _named()
    assert packed.slug(NAMES[1]) == packed.slug(NAMES[2])                                   # two names, one slug: distinct files all the same
    assert all(packed.slug(n) == cli._slug(n) for n in NAMES + ["", "//", "a b/c.d"])       # wq's slug
    meta = {NAMES[0]: {"size_model_bytes": 12.5, "metric_value": 0.9991}}
    index = packed.save_dir(tmp_path / "d", {n: pt for n, (_x, pt) in named.items()}, meta=meta, run={"algorithm": "by hand"})
    on_disk = json.loads((tmp_path / "d" / "index.json").read_text())
    assert on_disk == index and on_disk["format_version"] == packed.FORMAT_VERSION and on_disk["run"] == {"algorithm": "by hand"}
    assert list(on_disk["tensors"]) == NAMES and len({e["file"] for e in on_disk["tensors"].values()}) == len(NAMES)
    assert on_disk["tensors"][NAMES[0]]["file"] == "model.layers.0.attn.q.weight.npz"
    for name, (x, pt) in named.items():
        e = on_disk["tensors"][name]
        assert (tmp_path / "d" / e["file"]).is_file()
        assert e["shape"] == list(x.shape) and e["counts"] == pt.counts() and e["nbytes"] == pt.nbytes and e["total_bytes"] == pt.total_bytes
    assert on_disk["tensors"][NAMES[0]]["size_model_bytes"] == 12.5 and "metric_value" not in on_disk["tensors"][NAMES[1]]
    back = packed.load_dir(tmp_path / "d")
    assert list(back) == NAMES
    for name, (x, pt) in named.items():
        b = back[name]
        assert b.shape == pt.shape and np.array_equal(b.map, pt.map) and np.array_equal(b.offsets, pt.offsets) and np.array_equal(b.data, pt.data)
        assert np.array_equal(np.asarray(packed.unpack(b)).view(np.uint32), expected_bits(x, pt.map))
    with pytest.raises(hb.MtqError, match="may not set"):
        packed.save_dir(tmp_path / "e", {NAMES[0]: named[NAMES[0]][1]}, meta={NAMES[0]: {"nbytes": 1}})


def test_load_dir_checks_the_index_against_the_files(tmp_path):
    named = {n: pt for n, (_x, pt) in _named().items()}
    d = tmp_path / "d"
    packed.save_dir(d, named)
    text = (d / "index.json").read_text()
    index = json.loads(text)

    def with_index(doc):
        (d / "index.json").write_text(json.dumps(doc))

    for version in (packed.FORMAT_VERSION + 1, None):
        with_index({**index, "format_version": version})
        with pytest.raises(hb.MtqError, match="version"):
            packed.load_dir(d)
    with_index({k: v for k, v in index.items() if k != "format_version"})
    with pytest.raises(hb.MtqError, match="version"):
        packed.load_dir(d)
    with_index(index)
    assert list(packed.load_dir(d)) == NAMES
    # a stream shorter than the index says: the file re-written with its last blob gone, and an index that promises more than the file
    f = d / index["tensors"][NAMES[1]]["file"]
    with np.load(f) as z:
        fields = {k: z[k] for k in z.files}
    np.savez(f, **{**fields, "data": fields["data"][:-64]})
    with pytest.raises(hb.MtqError, match="stream"):
        packed.load_dir(d)
    np.savez(f, **fields)
    more = json.loads(text)
    more["tensors"][NAMES[1]]["nbytes"] += 64
    with_index(more)
    with pytest.raises(hb.MtqError, match="stream holds .* the index says"):
        packed.load_dir(d)
    other = json.loads(text)
    other["tensors"][NAMES[0]]["shape"] = [50, 70]
    with_index(other)
    with pytest.raises(hb.MtqError, match="shape"):
        packed.load_dir(d)
    with_index(index)
    f.unlink()
    with pytest.raises(hb.MtqError, match="missing"):
        packed.load_dir(d)
    (d / "index.json").unlink()
    with pytest.raises(hb.MtqError, match="index.json is missing"):
        packed.load_dir(d)


def pack_model_script():
    spec = importlib.util.spec_from_file_location("pack_model", ROOT / "scripts" / "pack_model.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pack_model_on_the_emulation_backend(tmp_path, capsys):
    script = pack_model_script()
    out = tmp_path / "packed"
    assert script.main(["synthetic:tiny", "--compression-config", str(GREEDY), "--out-dir", str(out), "--backend", "emulation", "--verify"]) == 0
    text = capsys.readouterr().out
    assert "verify: ok (5 tensors" in text and "total packed bytes" in text and "size-model bytes" in text and "MISMATCH" not in text
    index = json.loads((out / "index.json").read_text())
    run = index["run"]
    assert run["algorithm"] == "mixed-tile-greedy" and run["seed_source"] == "random" and run["params"]["seed"] == run["seed"] != 0
    back = packed.load_dir(out)
    idx = model_source.build_model_index("synthetic:tiny")
    names = model_source.resolve_selected_tensors(idx, None)
    assert list(back) == names and len(names) == 5
    algo = create_algorithm(run["algorithm"], run["params"])            # the example config draws its seed: the index says which
    for name in names:
        x = np.asarray(idx.load(name).float().numpy(), dtype=np.float32)
        res = algo.run(xf=x, formats=run["formats"], quantizer=Quantizer("emulation"), cache=CacheContext(tmp_path / "c", name, "emulation", True, "t"))[0]
        pt = back[name]
        assert np.array_equal(pt.map, res.meta["assignment"]) and pt.shape == x.shape
        y = np.asarray(packed.unpack(pt), dtype=np.float32)
        assert y.shape == x.shape and np.array_equal(y.view(np.uint32), np.ascontiguousarray(res.y, dtype=np.float32).view(np.uint32))
        e = index["tensors"][name]
        assert e["route"] == "per-tensor" and e["verified"] is True and e["nbytes"] == pt.nbytes
        assert e["size_model_bytes"] == pytest.approx(res.tile_bytes) and e["metric_value"] == pytest.approx(res.meta["metric_value"])
        assert f"{name} {x.shape} per-tensor: packed bytes {pt.nbytes} " in text
    # a filter and a limit, as wq takes them
    assert script.main(["synthetic:tiny", "attn", "--limit", "1", "--compression-config", str(GREEDY), "--out-dir", str(tmp_path / "one")]) == 0
    assert list(packed.load_dir(tmp_path / "one")) == ["model.layers.0.attn.k.weight"]


def test_pack_model_reports_a_mismatch(tmp_path, capsys):
    script = pack_model_script()
    real = script.packed.unpack

    def flipped(pt, **kw):
        pt.data = pt.data.copy()
        pt.data[100] ^= 0x10
        return real(pt, **kw)

    script.packed.unpack = flipped
    try:
        rc = script.main(["synthetic:tiny", "model.layers.0.attn.k.weight", "--compression-config", str(GREEDY), "--out-dir", str(tmp_path / "p"), "--verify"])
    finally:
        script.packed.unpack = real
    text = capsys.readouterr().out
    assert rc == 2 and "model.layers.0.attn.k.weight" in text and "MISMATCH" in text


def test_pack_model_refuses_what_it_cannot_pack(tmp_path, capsys):
    script = pack_model_script()
    assert script.main(["synthetic:tiny", "--compression-config", str(TRANSPOSED), "--out-dir", str(tmp_path / "t")]) == 1
    assert "row layout" in capsys.readouterr().out and not (tmp_path / "t").exists()
    (tmp_path / "none.json").write_text('{"algorithm": "none"}')
    assert script.main(["synthetic:tiny", "--compression-config", str(tmp_path / "none.json"), "--out-dir", str(tmp_path / "n")]) == 1
    assert "writes no tile map" in capsys.readouterr().out
    assert script.main(["synthetic:tiny", "no-such-tensor", "--compression-config", str(GREEDY), "--out-dir", str(tmp_path / "m")]) == 1
    assert "No tensors matched" in capsys.readouterr().out


def test_batched_c_abi_argument_errors_need_no_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    big = 1 << 20
    limit = 0xFFFFFFFF // 32
    assert hb.PACKED_BATCH_MAX_TILES == limit
    for name in ("mtq_packed_offsets_batched", "mtq_pack_tiles_batched", "mtq_unpack_tiles_batched"):
        assert hb.SIGNATURES[name][2] is True and name in hb.OPTIONAL_EXPORTS

    def call(fn, ok, **kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return fn(*args)

    # offsets: maps, count, tiles, offsets, bases, bad, stream
    oko = (p, 3, 6, p, p, p, None)
    for null in (0, 3, 4, 5):
        assert call(L.mtq_packed_offsets_batched, oko, **{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    for count in (0, -1):
        assert call(L.mtq_packed_offsets_batched, oko, a1=count) == -1 and b"count" in L.mtq_last_error()
    for tiles in (0, -5):
        assert call(L.mtq_packed_offsets_batched, oko, a2=tiles) == -1 and b"tiles" in L.mtq_last_error()
    assert call(L.mtq_packed_offsets_batched, oko, a2=limit + 1) == -1 and b"32-bit units" in L.mtq_last_error()
    assert call(L.mtq_packed_offsets_batched, oko, a1=1 << 40, a2=limit) == -1 and b"batch" in L.mtq_last_error()

    # pack: x, in_dtype, count, rows, cols, ld, stride, maps, offsets, bases, out, out_bytes, stream
    okp = (p, 0, 3, 64, 64, 64, 64 * 64, p, p, p, p, big, None)
    for null in (0, 7, 8, 9, 10):
        assert call(L.mtq_pack_tiles_batched, okp, **{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a1=7) == -1 and b"in_dtype" in L.mtq_last_error()
    for count in (0, -2):
        assert call(L.mtq_pack_tiles_batched, okp, a2=count) == -1 and b"count" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a3=0) == -1 and call(L.mtq_pack_tiles_batched, okp, a4=-1) == -1
    assert call(L.mtq_pack_tiles_batched, okp, a3=1 << 19, a4=1 << 19, a5=1 << 19) == -1 and b"32-bit units" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a5=63) == -1 and b"ld < cols" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a6=64 * 63 + 63) == -1 and b"stride" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a11=3 * 4 * 320 - 1) == -1 and b"smaller than the streams" in L.mtq_last_error()
    assert call(L.mtq_pack_tiles_batched, okp, a10=p + 8) == -1 and b"aligned" in L.mtq_last_error()

    # unpack: packed, packed_bytes, maps, offsets, bases, count, rows, cols, y, out_dtype, ldy, stride, stream
    oku = (p, big, p, p, p, 3, 64, 64, p, 1, 64, 64 * 64, None)
    for null in (0, 2, 3, 4, 8):
        assert call(L.mtq_unpack_tiles_batched, oku, **{f"a{null}": None}) == -1 and b"null" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a9=2) == -1 and b"out_dtype" in L.mtq_last_error()
    for count in (0, -2):
        assert call(L.mtq_unpack_tiles_batched, oku, a5=count) == -1 and b"count" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a6=0) == -1 and call(L.mtq_unpack_tiles_batched, oku, a7=-1) == -1
    assert call(L.mtq_unpack_tiles_batched, oku, a6=1 << 19, a7=1 << 19, a10=1 << 19) == -1 and b"32-bit units" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a10=63) == -1 and b"ldy < cols" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a11=64 * 63 + 63) == -1 and b"stride" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a1=3 * 4 * 320 - 1) == -1 and b"smaller than the streams" in L.mtq_last_error()
    assert call(L.mtq_unpack_tiles_batched, oku, a0=p + 4) == -1 and b"aligned" in L.mtq_last_error()
    # a batch of one has no second matrix: its stride means nothing
    import torch

    if not torch.cuda.is_available():     # everything in order: only the device is missing
        assert call(L.mtq_packed_offsets_batched, oko) == -3 and call(L.mtq_pack_tiles_batched, okp) == -3 and call(L.mtq_unpack_tiles_batched, oku) == -3
        assert call(L.mtq_pack_tiles_batched, okp, a2=1, a6=0) == -3 and call(L.mtq_unpack_tiles_batched, oku, a5=1, a11=0) == -3


class _OnDevice:
    """A host tensor that passes for a device tensor in the binding's checks, with a null pointer (tests/test_packed_host.py): a call that
    got past every check is refused by the library's own null check, never launched."""

    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return 0


def test_batched_wrappers_check_what_they_dereference():
    import torch

    def D(*shape, dtype=torch.uint8):
        return _OnDevice(torch.zeros(shape, dtype=dtype))

    count, rows, cols, tiles = 3, 64, 96, 6
    maps, offs, bases = D(count, tiles, dtype=torch.int8), D(count, tiles + 1, dtype=torch.int32), D(count + 1, dtype=torch.int64)
    x = _OnDevice(torch.zeros((count, rows, cols), dtype=torch.bfloat16))
    arena = D(count * tiles * 2048)
    with pytest.raises(hb.MtqError, match="positive"):
        hb.packed_offsets_device(maps, 0, tiles)
    with pytest.raises(hb.MtqError, match="32-bit units"):
        hb.packed_offsets_device(maps, 1, hb.PACKED_BATCH_MAX_TILES + 1)
    with pytest.raises(hb.MtqError, match="device maps"):
        hb.packed_offsets_device(maps, count, tiles + 1)
    with pytest.raises(hb.MtqError, match="device maps"):
        hb.packed_offsets_device(torch.zeros((count, tiles), dtype=torch.int8), count, tiles)      # host memory
    for bad, msg in ((torch.zeros((count, rows, cols)), "device tensor"), (_OnDevice(torch.zeros((rows, cols))), "3-D"),
                     (_OnDevice(torch.zeros((count, rows, 2 * cols))[:, :, ::2]), "contiguous rows"), (_OnDevice(torch.zeros((count, rows, cols)).half()), "bfloat16 or float32")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles_batched(bad, maps, offs, bases, arena)
    for tables, msg in (((D(count, tiles - 1, dtype=torch.int8), offs, bases), "device maps"), ((maps, D(count, tiles, dtype=torch.int32), bases), "device offsets"),
                        ((maps, offs, D(count, dtype=torch.int64)), "device bases"), ((maps, offs, D(count + 1, dtype=torch.int32)), "device bases")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles_batched(x, *tables, arena)
        with pytest.raises(hb.MtqError, match=msg):
            hb.unpack_tiles_batched(arena, *tables, count, rows, cols, out=D(count, rows, cols, dtype=torch.float32))
    for out, msg in ((D(count * tiles * 320 - 1), "out"), (torch.zeros(count * tiles * 2048, dtype=torch.uint8), "out"), (D(count * tiles * 2048, dtype=torch.int8), "out")):
        with pytest.raises(hb.MtqError, match=msg):
            hb.pack_tiles_batched(x, maps, offs, bases, out)
    with pytest.raises(hb.MtqError, match="null argument"):                    # every check passed: the library's turn
        hb.pack_tiles_batched(x, maps, offs, bases, arena, stream=None)
    y = D(count, rows, cols, dtype=torch.float32)
    with pytest.raises(hb.MtqError, match="data"):
        hb.unpack_tiles_batched(D(count * tiles * 320 - 1), maps, offs, bases, count, rows, cols, out=y)
    with pytest.raises(hb.MtqError, match="output type"):
        hb.unpack_tiles_batched(arena, maps, offs, bases, count, rows, cols, dtype=torch.float16, out=y)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.unpack_tiles_batched(arena, maps, offs, bases, count, rows, cols, dtype=torch.bfloat16, out=y)
    with pytest.raises(hb.MtqError, match="out must be"):
        hb.unpack_tiles_batched(arena, maps, offs, bases, count, rows, cols, out=torch.zeros((count, rows, cols)))
    with pytest.raises(hb.MtqError, match="null argument"):
        hb.unpack_tiles_batched(arena, maps, offs, bases, count, rows, cols, out=y, stream=None)
