"""GPU: packed.embedding (packed_gather_rows_kernel / packed_gather_columns_kernel, csrc/mtq_packed_gather.hip) against the NumPy decoder's
table indexed by the ids, bit for bit: a gather has no rounding to tolerate, and with a scale the float64 product of two float32 values
is exact, so its rounding to float32 and from there to bf16 is the one answer.

(vocab, hidden): (70, 72) a ragged last tile row and a last tile whose second group is all padding; (33, 8) hidden below one group;
(96, 2080) hidden past one wave's 1024 columns, with a tail; (64, 4128) five units a row, so a wave's four units in flight cross tokens.
Maps: random over the four codes (one row crosses all formats) and each pure format.  The ids hold 0, 31, 32, vocab - 1, duplicates,
-1, vocab and 2^40 (int64), as a (3, 5) tensor, a strided view and a single token, with id_first 0 and 32."""
import copy
import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb, packed
from tests.inputs import gen
from tests.packed_cases import TILE_BYTES, random_map, uniform_map

pytestmark = pytest.mark.gpu
SHAPES = ((70, 72), (33, 8), (96, 2080), (64, 4128))
MAPS = ("random", 0, 1, 2, 3)
GRID_UNITS = 2048 * 4 * 4          # the launch's cap: 2048 workgroups of four waves with four units each


@functools.lru_cache(maxsize=None)
def _case(shape, kind, stored):
    """(the packed tensor as `stored` has it, the (vocab, hidden) float32 table the NumPy decoder gives for it)."""
    vocab, hidden = shape
    w = gen("heavy_f32", vocab + hidden, shape)
    grid = (hidden, vocab) if stored == "transpose" else shape
    amap = random_map(grid, 7) if kind == "random" else uniform_map(grid, kind)
    if stored == "transpose":
        pt = packed.pack_transposed(w, amap)
        return pt, packed.unpack_transposed(pt, backend="emulation")
    pt = packed.pack(w, amap)
    return pt, packed.unpack(pt, backend="emulation")


def _want(table, ids, id_first=0, scale=None, dtype="float32"):
    ids = np.asarray(ids, dtype=np.int64) - id_first
    inside = (ids >= 0) & (ids < table.shape[0])
    rows = np.where(inside[..., None], table[np.where(inside, ids, 0)], np.float32(0))
    if scale is not None:
        rows = (rows.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)
    t = torch.from_numpy(np.ascontiguousarray(rows))
    return _bits(t if dtype == "float32" else t.to(torch.bfloat16))     # without a scale every value is a bf16 value: exact


def _bits(t) -> np.ndarray:
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _ids(vocab, dtype):
    far = 2 ** 40 if dtype == torch.int64 else vocab + 7
    return torch.tensor([0, 31, 32, vocab - 1, 5, 5, -1, vocab, far, 1, vocab - 1, 33 % vocab, 2, 0, 31], dtype=dtype).reshape(3, 5)


@pytest.mark.parametrize("stored", packed.MOE_STORED)
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_gather_is_the_decoders_rows_bit_for_bit(shape, kind, stored):
    pt, table = _case(shape, kind, stored)
    vocab, hidden = shape
    scale = float(np.float32(np.sqrt(hidden)))
    for id_dtype in (torch.int32, torch.int64):
        ids = _ids(vocab, id_dtype)
        for dtype in ("float32", "bfloat16"):
            for id_first, sc in ((0, None), (32, None), (0, scale)):
                got = packed.embedding(ids.cuda(), pt, out_dtype=dtype, stored=stored, scale=sc, id_first=id_first, backend="hip")
                assert tuple(got.shape) == (3, 5, hidden)
                assert np.array_equal(_bits(got), _want(table, ids.numpy(), id_first, sc, dtype)), (id_dtype, dtype, id_first, sc)
    wide = torch.stack([_ids(vocab, torch.int64), torch.zeros((3, 5), dtype=torch.int64)], dim=-1).cuda()[..., 0]      # a strided view
    assert not wide.is_contiguous()
    one = torch.tensor([vocab - 1], dtype=torch.int32).cuda()
    for ids in (wide, one):
        got = packed.embedding(ids, pt, stored=stored, backend="hip")
        again = packed.embedding(ids, pt, stored=stored, backend="hip")
        assert np.array_equal(_bits(got), _want(table, ids.cpu().numpy(), dtype="bfloat16")) and np.array_equal(_bits(got), _bits(again))


@pytest.mark.parametrize("stored", packed.MOE_STORED)
def test_more_tokens_than_the_grid_holds_at_once(stored):
    pt, table = _case((33, 8), "random", stored)
    ids = torch.from_numpy(np.random.default_rng(3).integers(-2, 36, size=GRID_UNITS + 37)).cuda()
    got = packed.embedding(ids, pt, out_dtype="float32", stored=stored, backend="hip")
    assert np.array_equal(_bits(got), _want(table, ids.cpu().numpy()))


@pytest.mark.parametrize("stored", packed.MOE_STORED)
def test_out_as_a_column_window_keeps_the_rest_of_the_buffer(stored):
    pt, table = _case((70, 72), "random", stored)
    ids = _ids(70, torch.int64).reshape(-1)
    for dtype, fill in (("bfloat16", -3.0), ("float32", -3.0)):
        buf = torch.full((15, 72 + 24), fill, dtype=packed._torch_dtype(dtype), device="cuda")
        out = packed.embedding(ids.cuda(), pt, out_dtype=dtype, stored=stored, backend="hip", out=buf[:, 3:75])      # an unaligned first element
        assert out.data_ptr() == buf[:, 3:75].data_ptr() and np.array_equal(_bits(out), _want(table, ids.numpy(), dtype=dtype))
        rest = torch.cat([buf[:, :3], buf[:, 75:]], dim=1)
        assert bool((rest == fill).all())


@pytest.mark.parametrize("stored", packed.MOE_STORED)
def test_a_blob_past_packed_bytes_reads_as_zeros(stored):
    pt, table = _case((70, 72), "random", stored)
    pt = copy.copy(pt)
    data = packed._device_data(pt)
    last = pt.map.size - 1
    cut = int(pt.offsets[last]) * 64 + TILE_BYTES[int(pt.map.reshape(-1)[last])] - 64         # 64 bytes short of the end of the last tile
    assert pt.map.size * TILE_BYTES[3] <= cut < pt.nbytes == data.numel()                      # the entry refuses less; the buffer stays whole
    short = copy.copy(pt.tables())
    short.nbytes = cut
    left = table.copy()
    left[64:, 64:] = 0                                                                         # the last tile, in the table's orientation
    assert np.count_nonzero(left != table) > 0
    ids = torch.tensor([0, 63, 64, 69, 33], dtype=torch.int32).cuda()
    got = hb.packed_embedding(ids, data, short, pt.rows, pt.cols, stored=packed.MOE_STORED.index(stored), out_dtype=torch.float32)
    assert np.array_equal(_bits(got), _want(left, ids.cpu().numpy()))


def test_a_member_of_a_batch_is_read_from_its_slice_of_the_arena():
    x = np.stack([gen("heavy_f32", s, (70, 72)) for s in (1, 2, 3)])
    maps = np.stack([random_map((70, 72), s) for s in (4, 5, 6)])
    pts = packed.pack_batch(torch.from_numpy(x).cuda(), maps, backend="hip")
    ids = _ids(70, torch.int64)
    got = packed.embedding(ids.cuda(), pts[1], out_dtype="float32")
    assert np.array_equal(_bits(got), _want(packed.unpack(pts[1], backend="emulation"), ids.numpy()))
