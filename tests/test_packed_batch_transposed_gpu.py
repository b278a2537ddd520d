"""GPU: the batched transposed packed kernels (csrc/mtq_packed.hip) and packed.pack_batch_transposed / unpack_batch_transposed on the hip
backend.

  * pack: the arena is the emulation's, byte for byte, and each slice is what the single-tensor transposed kernel writes, for float32 and
    bf16 storage, ragged edges, 1 x n and n x 1 weights, every uniform map and random maps with every code; views that force the
    element-wise loads (an odd row pitch, a [::2] batch view at an unaligned address) and aligned views with a matrix stride, whose
    inner tiles take the 16-byte loads and whose edge tiles do not, with the edge inside a 16-byte piece; device maps give the arena host maps give; two
    calls give the same bytes over an arena filled beforehand;
  * unpack: float32 is K3T's bit for bit, bf16 its upper halves; nothing outside rows x cols is stored;
  * bounds: an arena one blob short keeps the last blob out and everything before it right;
  * the grid-stride loops: a batch of 2^22 + 5 weights of shape 1 x 1 is five waves more than the grid's cap of 2^20 workgroups of four
    holds, so both kernels take a second round: every tensor's word is the oracle's;
  * matmul on a tensor of the batch gives the bits it gives on the tensor packed alone; a transposed search pipeline's maps go to the
    pack and come back as K3T's reconstruction; scripts/pack_model.py --store-transposed on hip writes what it writes on emulation.

n != k throughout: a swapped axis cannot pass."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen
from tests.packed_cases import TILE_BYTES, expected_bits, specials, uniform_map
from tests.test_packed_batch_gpu import ROUND, _scalars
from tests.test_packed_batch_host import ROOT, pack_model_script
from tests.test_packed_batch_transposed_host import SHAPES, batch, transposed_maps
from tests.test_packed_gpu import bf16_valued_bits, dev

pytestmark = pytest.mark.gpu
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def batches():
    """(name, storage, float32 values (count, n, k), maps over the (k, n) grid) — computed once, shared, never written to."""
    out = []
    for name, _count, _n, _k in SHAPES:
        w, maps = batch(name)
        out.append((f"{name}-f32", "f32", w, maps))
        out.append((f"{name}-bf16", "bf16", bf16_valued_bits(w), maps))
    for code in range(4):
        out.append((f"1x32x32-{hb.MIXED_TILE_FORMATS[code]}", "f32", gen("heavy_f32", 90 + code, (1, 32, 32)), uniform_map((32, 32), code)[None]))
        out.append((f"3x70x100-{hb.MIXED_TILE_FORMATS[code]}", "bf16", bf16_valued_bits(np.stack([specials((70, 100), seed=31 + i) for i in range(3)])),
                    np.stack([uniform_map((100, 70), code)] * 3)))
    for _n, _s, w, _maps in out:
        w.setflags(write=False)
    return out


def _case(name):
    return next(b for b in batches() if b[0] == name)


@functools.lru_cache(maxsize=None)
def encoded(name):
    """The emulation's arena of a batch and the streams' lengths."""
    _n, _s, w, maps = _case(name)
    pts = packed.pack_batch_transposed(w, maps, backend="emulation")
    arena = packed.batch_of(pts).arena
    arena.setflags(write=False)
    return arena, [pt.nbytes for pt in pts]


def _arena(pts) -> np.ndarray:
    return packed.batch_of(pts).arena.cpu().numpy()


# ----------------------------------------------------------------------------- pack

@pytest.mark.parametrize("name", [b[0] for b in batches()])
def test_arena_is_the_emulations_byte_for_byte(name):
    _n, storage, w, maps = _case(name)
    want, sizes = encoded(name)
    count, n, k = w.shape
    wd = dev(w, storage)
    pts = packed.pack_batch_transposed(wd, maps, backend="hip")
    b = packed.batch_of(pts)
    g = _arena(pts)
    assert (b.count, b.rows, b.cols) == (count, k, n) and g.size == want.size == 64 * int(b.bases[count]) and b.arena.dtype == torch.uint8
    diff = np.flatnonzero(g != want)
    assert diff.size == 0, (name, diff[:8], g[diff[:8]], want[diff[:8]])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert np.array_equal(b.bases.astype(np.int64) * 64, starts)
    for i, pt in enumerate(pts):
        assert pt.on_device and pt.data.data_ptr() == b.arena.data_ptr() + starts[i] and pt.nbytes == sizes[i] and pt.shape == (k, n)
        assert np.array_equal(pt.map, maps[i]) and np.array_equal(pt.offsets, packed.offsets_of(maps[i]))
        alone = hb.pack_tiles_transposed(wd[i], hb.PackedTables.on_device(maps[i]))
        assert torch.equal(pt.data, alone), (name, i)                                   # the single-tensor kernel's bytes
        assert pt.tables().map_dev.data_ptr() == b.maps_dev[i].data_ptr()               # slices, no second upload
    from_device = packed.pack_batch_transposed(wd, torch.from_numpy(maps.copy()).cuda(), backend="hip")
    assert np.array_equal(_arena(from_device), g), name
    assert all(np.array_equal(a.map, c.map) and np.array_equal(a.offsets, c.offsets) for a, c in zip(from_device, pts))
    # two calls, the same bytes, whatever the arena held before: every byte is written
    again = torch.full((g.size,), FILL, dtype=torch.uint8, device="cuda")
    hb.pack_tiles_transposed_batched(wd, b.maps_dev, b.offsets_dev, b.bases_dev, again)
    assert np.array_equal(again.cpu().numpy(), g), name


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_views_are_read_in_place_on_either_load_path(storage):
    count, n, k = 3, 70, 100
    w = np.stack([specials((n, k), seed=41 + i) for i in range(2 * count)])
    w = w if storage == "f32" else bf16_valued_bits(w)
    maps = transposed_maps(count, n, k, 90)
    want = packed.batch_of(packed.pack_batch_transposed(w[::2], maps, backend="emulation")).arena
    esz = 4 if storage == "f32" else 2
    tdtype = dev(w[:1], storage).dtype
    # [:, :, :k] of a wider buffer with an odd row pitch: rows start at no aligned address, the loads are element-wise
    wide = torch.zeros((count, n, k + 9), dtype=tdtype, device="cuda")
    wide[:, :, :k] = dev(w[::2], storage)
    pitched = wide[:, :, :k]
    assert pitched.stride(1) == k + 9 and (pitched.stride(1) * esz) % 16 != 0 and not pitched.is_contiguous()
    assert np.array_equal(_arena(packed.pack_batch_transposed(pitched, maps, backend="hip")), want), storage
    # [::2] of a buffer that starts one element past an aligned address: no matrix is 16-byte aligned
    flat = torch.zeros(w.size + 8, dtype=tdtype, device="cuda")
    flat[1: 1 + w.size] = dev(w, storage).reshape(-1)
    view = flat[1: 1 + w.size].view(2 * count, n, k)[::2]
    assert view.data_ptr() % 16 == esz and view.stride(0) == 2 * n * k
    assert np.array_equal(_arena(packed.pack_batch_transposed(view, maps, backend="hip")), want), storage
    # the same [::2] view at an aligned address with an aligned pitch (104 elements): the 16-byte loads with a matrix stride in the
    # tiles that lie inside the matrix, element-wise loads in the edge tiles
    padded = torch.zeros((2 * count, n, 104), dtype=tdtype, device="cuda")
    padded[:, :, :k] = dev(w, storage)
    aligned = padded[::2, :, :k]
    assert aligned.data_ptr() % 16 == 0 and (aligned.stride(1) * esz) % 16 == 0 and (aligned.stride(0) * esz) % 16 == 0
    assert np.array_equal(_arena(packed.pack_batch_transposed(aligned, maps, backend="hip")), want), storage
    # an aligned view two columns narrower: the edge falls inside a 16-byte piece
    k2 = k - 2
    maps2 = transposed_maps(count, n, k2, 95)
    want2 = packed.batch_of(packed.pack_batch_transposed(w[::2, :, :k2], maps2, backend="emulation")).arena
    assert np.array_equal(_arena(packed.pack_batch_transposed(padded[::2, :, :k2], maps2, backend="hip")), want2), storage


# ----------------------------------------------------------------------------- unpack

@pytest.mark.parametrize("name", ["3x70x100-f32", "4x64x96-bf16", "2x33x31-f32", "2x1x40-bf16", "2x40x1-f32", "1x32x32-bfp4", "3x70x100-bfp2"])
def test_unpack_is_k3t_bit_for_bit(name):
    _n, storage, w, maps = _case(name)
    count, n, k = w.shape
    wd = dev(w, storage)
    pts = packed.pack_batch_transposed(wd, maps, backend="hip")
    y = packed.unpack_batch_transposed(pts, backend="hip")
    assert y.dtype == torch.float32 and tuple(y.shape) == (count, n, k)
    yb = y.cpu().numpy().view(np.uint32)
    for i in range(count):
        k3t = hb.apply_assignment_transposed(wd[i], maps[i]).cpu().numpy().view(np.uint32)
        assert np.array_equal(yb[i], k3t), (name, i, np.argwhere(yb[i] != k3t)[:4])
        assert np.array_equal(yb[i], np.ascontiguousarray(expected_bits(np.ascontiguousarray(w[i].T), maps[i]).T)), (name, i)      # the oracle
        assert np.array_equal(packed.unpack_transposed(pts[i], backend="hip").cpu().numpy().view(np.uint32), yb[i]), (name, i)  # the slice alone
    half = packed.unpack_batch_transposed(pts, backend="hip", dtype="bfloat16")
    assert half.dtype == torch.bfloat16
    assert np.array_equal(half.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << np.uint32(16), yb), name
    # the same list as what it is, a batch of (k, n) tensors: the transposes
    assert np.array_equal(packed.unpack_batch(pts, backend="hip").cpu().numpy().view(np.uint32), yb.transpose(0, 2, 1)), name
    # a list that is not the whole batch in order goes tensor by tensor, to the same bits
    assert np.array_equal(packed.unpack_batch_transposed(pts[::-1], backend="hip").cpu().numpy().view(np.uint32), yb[::-1]), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unpack_stores_nothing_outside_the_matrices(dtype):
    _n, storage, w, maps = _case("3x70x100-f32")
    count, n, k = w.shape
    pts = packed.pack_batch_transposed(dev(w, storage), maps, backend="hip")
    b = packed.batch_of(pts)
    want = packed.unpack_batch_transposed(pts, backend="hip", dtype="float32" if dtype == torch.float32 else "bfloat16")
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    filled = int(torch.full((want.element_size(),), FILL, dtype=torch.uint8).view(ints))      # an element of 0xA5 bytes
    for r0, c0 in ((0, 0), (1, 3)):
        big = torch.full((count, n + 7, (k + 12) * want.element_size()), FILL, dtype=torch.uint8, device="cuda").view(dtype)
        assert tuple(big.shape) == (count, n + 7, k + 12)
        out = big[:, r0: r0 + n, c0: c0 + k]
        hb.unpack_tiles_transposed_batched(b.arena, b.maps_dev, b.offsets_dev, b.bases_dev, count, n, k, dtype, out=out)
        assert torch.equal(out.contiguous().view(ints), want.view(ints))
        outside = torch.ones(big.shape, dtype=torch.bool, device="cuda")
        outside[:, r0: r0 + n, c0: c0 + k] = False
        assert bool((big.view(ints)[outside] == filled).all()), (dtype, r0, c0)


# ----------------------------------------------------------------------------- bounds

def test_an_arena_one_blob_short_keeps_the_last_blob_out():
    """Not a fault: the kernels check every blob against the arena's length themselves."""
    _n, storage, w, maps = _case("3x70x100-f32")
    want, _sizes = encoded("3x70x100-f32")
    count, n, k = w.shape
    tiles = maps[0].size
    last = TILE_BYTES[int(maps[-1].reshape(-1)[-1])]
    md = torch.from_numpy(maps.reshape(count, tiles)).cuda()
    offsets, bases, _bad = hb.packed_offsets_device(md, count, tiles)
    arena = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
    assert want.size - last >= count * tiles * TILE_BYTES[3]                              # the entry's own lower bound still holds
    wd = dev(w, storage)
    for short in (last, 1):                                                                # one blob short, and one byte short of that blob
        arena.fill_(FILL)
        hb.pack_tiles_transposed_batched(wd, md, offsets, bases, arena[: want.size - short])
        g = arena.cpu().numpy()
        assert np.array_equal(g[: want.size - last], want[: want.size - last]) and np.all(g[want.size - last:] == FILL), short
    # unpack of the short arena stores nothing for that tile: the last tile of the (k, n) grid, rows 64.. and columns 96.. of W
    y = torch.full(w.shape, -7.0, dtype=torch.float32, device="cuda")
    arena[: want.size] = torch.from_numpy(np.array(want)).cuda()
    hb.unpack_tiles_transposed_batched(arena[: want.size - last], md, offsets, bases, count, n, k, out=y)
    yb = y.cpu().numpy()
    full = np.stack([np.ascontiguousarray(expected_bits(np.ascontiguousarray(w[i].T), maps[i]).T) for i in range(count)])
    in_last = np.zeros(w.shape, dtype=bool)
    in_last[-1, 64:, 96:] = True
    assert np.array_equal(yb.view(np.uint32)[~in_last], full[~in_last]) and np.all(yb[in_last] == -7.0)


# ----------------------------------------------------------------------------- the grid-stride loops' second round

@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_the_grid_stride_loops_take_a_second_round(storage):
    """tests/test_packed_batch_gpu.py's batch of 1 x 1 tensors (a 1 x 1 weight is its own transpose) through the transposed kernels, whose
    launch cap is the row kernels': ROUND waves to a round."""
    count = ROUND + 5
    u = _scalars(storage)
    carrier = np.zeros((64, 16), dtype=np.uint32)
    carrier[:, 0] = u
    table = np.stack([expected_bits(carrier.view(np.float32), uniform_map((64, 16), c))[:, 0] for c in range(4)], axis=1)
    rng = np.random.default_rng(4243)
    codes = rng.choice(4, size=count, p=[1 / 64, 21 / 64, 21 / 64, 21 / 64]).astype(np.int8)     # bf16 blobs (2048 B) are rare
    codes[[0, ROUND - 1, ROUND, ROUND + 4]] = [0, 1, 2, 3]
    ids = np.arange(count) % 64
    units = np.asarray(TILE_BYTES)[codes] // 64
    assert 64 * int(units.sum()) < 3 * 2 ** 30
    wd = dev(u.view(np.float32)[ids].reshape(count, 1, 1), storage)
    maps_dev = torch.from_numpy(codes.reshape(count, 1)).cuda()
    offsets, bases_dev, bad = hb.packed_offsets_device(maps_dev, count, 1)
    assert not bool(bad.any())
    bases = bases_dev.cpu().numpy().view(np.uint64)
    arena = torch.empty((64 * int(bases[count]),), dtype=torch.uint8, device="cuda")
    arena[64 * int(bases[ROUND]):] = FILL                                                      # what a kernel without a second round leaves
    hb.pack_tiles_transposed_batched(wd, maps_dev, offsets, bases_dev, arena)
    for i in (0, ROUND - 1, ROUND, ROUND + 4):
        value = u.view(np.float32)[ids[i]].reshape(1, 1)
        want = packed.pack_transposed(value, np.array([[codes[i]]], dtype=np.int8), backend="emulation").data
        got = arena[64 * int(bases[i]): 64 * int(bases[i + 1])].cpu().numpy()
        assert np.array_equal(got, want), (storage, i, np.flatnonzero(got != want)[:8])
    want_dev = torch.from_numpy(table.view(np.int32)).cuda()[torch.from_numpy(ids).cuda(), maps_dev.reshape(-1).long()]
    y = torch.full((count, 1, 1), -7.0, dtype=torch.float32, device="cuda")
    hb.unpack_tiles_transposed_batched(arena, maps_dev, offsets, bases_dev, count, 1, 1, torch.float32, out=y)
    wrong = (y.view(torch.int32).reshape(-1) != want_dev).nonzero().reshape(-1)
    assert wrong.numel() == 0, (storage, "tensors", wrong[:8].tolist(), "of", count, "; the second round starts at", ROUND)


# ----------------------------------------------------------------------------- the tensors of a batch are full citizens

def test_matmul_on_a_batch_product_is_matmul_on_the_tensor_alone():
    count, n, k, m = 2, 96, 64, 40
    w = np.stack([gen("heavy_bf16", 3 + i, (n, k)) for i in range(count)])
    maps = transposed_maps(count, n, k, 6)
    wd = dev(w, "bf16")
    pts = packed.pack_batch_transposed(wd, maps, backend="hip")
    x = dev(gen("normal_bf16", 4, (m, k)) * 64, "bf16")
    bias = torch.from_numpy(gen("normal_f32", 5, (n,))).cuda()
    for i, pt in enumerate(pts):
        alone = packed.pack_transposed(wd[i], maps[i], backend="hip")
        assert torch.equal(pt.data, alone.data) and pt.data.data_ptr() % 64 == 0
        for out_dtype in ("float32", "bfloat16"):
            ints = torch.int32 if out_dtype == "float32" else torch.int16
            got = packed.matmul(x, pt, bias=bias, out_dtype=out_dtype)
            assert tuple(got.shape) == (m, n)
            assert torch.equal(got.view(ints), packed.matmul(x, alone, bias=bias, out_dtype=out_dtype).view(ints)), (i, out_dtype)
        for kernel, rows in (("skinny", 5), ("auto", m)):
            assert torch.equal(packed.matmul(x[:rows], pt, bias=bias, kernel=kernel).view(torch.int32),
                               packed.matmul(x[:rows], alone, bias=bias, kernel=kernel).view(torch.int32)), (i, kernel)
        assert torch.equal(packed.matmul_wide(x, pt, bias=bias).view(torch.int32), packed.matmul_wide(x, alone, bias=bias).view(torch.int32)), i
        layer = packed.PackedMatmul(pt, bias=bias)
        assert torch.equal(layer(x).view(torch.int32), packed.matmul(x, alone, bias=bias, kernel="auto").view(torch.int32)), i


def test_a_transposed_pipelines_maps_go_to_the_pack_and_come_back_as_k3t():
    from quantization_analysis_amd.pipeline import GreedyPipeline

    x3d = dev(np.stack([gen("heavy_bf16", 70 + i, (64, 96)) for i in range(3)]), "bf16")
    with GreedyPipeline(hb.MIXED_TILE_FORMATS, "pcc", 0.999, 123, chunk=3, layout="transpose") as pipe:
        results = pipe.run(x3d)
    maps = np.stack([r.assignment for r in results])
    assert maps.shape == (3, 3, 2)                                                             # over the (96, 64) transposes
    pts = packed.pack_batch_transposed(x3d, maps, backend="hip")
    y = packed.unpack_batch_transposed(pts, backend="hip")
    want = hb.apply_assignment_transposed(x3d, maps)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert [pt.counts() for pt in pts] == [r.counts for r in results]


# ----------------------------------------------------------------------------- the script

def test_pack_model_store_transposed_on_hip_writes_what_the_emulation_writes(tmp_path, capsys):
    script = pack_model_script()
    cfg = str(ROOT / "compression_configs" / "compression_config.mixed_tile_greedy_transpose.example.json")
    base = ["synthetic:tiny", "--compression-config", cfg, "--store-transposed", "--verify"]
    assert script.main(base + ["--out-dir", str(tmp_path / "hip"), "--backend", "hip"]) == 0
    text = capsys.readouterr().out
    assert "verify: ok (5 tensors" in text and "MISMATCH" not in text
    index = packed.read_index(tmp_path / "hip")
    assert script.main(base + ["--out-dir", str(tmp_path / "emu"), "--backend", "emulation"]) == 0
    hip, emu = packed.load_dir(tmp_path / "hip"), packed.load_dir(tmp_path / "emu")
    assert list(hip) == list(emu) and len(hip) == 5
    for name in hip:
        a, b = hip[name], emu[name]
        assert a.shape == b.shape and np.array_equal(a.map, b.map) and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.data, b.data), name
        assert (tmp_path / "hip" / index["tensors"][name]["file"]).read_bytes() == (tmp_path / "emu" / index["tensors"][name]["file"]).read_bytes(), name
    routes = {name: e["route"] for name, e in index["tensors"].items()}
    assert routes["model.layers.0.norm.weight"] == "per-tensor" and sorted(routes.values()).count("batched") == 4      # the vector alone goes one by one
    assert all(e["verified"] is True and e["stored"] == "transpose" for e in index["tensors"].values())
