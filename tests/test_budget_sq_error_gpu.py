"""mtq_tile_sq_error_batched: bit for bit the e_w of mtq_tile_error_tables for every matrix of a batch (bf16 and float32, whole and
ragged shapes, a strided batch view), and on inputs whose sums are exact in any order (tests/test_calibration_exact_host.py) bit for
bit the emulation table too."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from tests.test_calibration_exact_host import tables_int, tables_weight

pytestmark = pytest.mark.gpu
SHAPES = [(96, 160), (70, 100)]
COUNT = 3


def _batch(rows, cols, dtype, strided, seed=0):
    """(count, rows, cols) device tensor; strided: a view into a wider, taller buffer (ld > cols, stride(0) > rows · ld, an odd column
    offset, so the element-wise load path runs as well)."""
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(seed * 7919 + rows * 31 + cols)
    if not strided:
        x = (torch.randn((COUNT, rows, cols), generator=g, device="cuda") * 0.05).to(dtype)
        assert x.is_contiguous()
        return x
    base = (torch.randn((COUNT, rows + 3, cols + 9), generator=g, device="cuda") * 0.05).to(dtype)
    x = base[:, 1: 1 + rows, 3: 3 + cols]
    assert x.stride() == ((rows + 3) * (cols + 9), cols + 9, 1) and not x.is_contiguous()
    return x


def _per_matrix(x):
    tw = -(-x.shape[2] // 32)
    h = torch.zeros((tw, 32, 32), dtype=torch.float64, device=x.device)
    return torch.stack([hb.tile_error_tables(x[b], h, want_weight=True)[1] for b in range(x.shape[0])])


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_batched_table_equals_the_per_matrix_tables_bit_for_bit(rows, cols, dtype, strided):
    x = _batch(rows, cols, dtype, strided)
    got = hb.tile_sq_error_batched(x)
    th, tw = hb.tiles_hw(rows, cols)
    assert got.shape == (COUNT, th * tw, 4) and got.dtype == torch.float64
    want = _per_matrix(x)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert bool((got[:, :, 3] > 0).all()) and bool((got[:, :, 0] == 0).all()) == (dtype == torch.bfloat16)
    one = hb.tile_sq_error_batched(x[1])                                       # a 2-D tensor is a batch of one
    assert torch.equal(one[0].view(torch.int64), want[1].view(torch.int64))
    # close to the float64 emulation (the exact comparison is below)
    emu = bm.tile_error_tables_emulation(x[2].float().cpu().numpy(), np.zeros((tw, 32, 32)))[1]
    assert np.allclose(got[2].cpu().numpy(), emu, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("wdt", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_exact_sum_inputs_equal_the_emulation_bit_for_bit(rows, cols, wdt):
    torch.cuda.set_device(0)
    ws = [tables_weight(rows, cols, seed) for seed in range(COUNT)]             # (rows, cols + 5): the view [:, 2 : 2 + cols] is the matrix
    dtype = torch.bfloat16 if wdt == "bf16" else torch.float32
    base = torch.stack([torch.from_numpy(w) for w in ws]).to(dtype).cuda()
    assert all(np.array_equal(base[b].float().cpu().numpy().view(np.uint32), ws[b].view(np.uint32)) for b in range(COUNT))
    x = base[:, :, 2: 2 + cols]
    got = hb.tile_sq_error_batched(x).cpu().numpy()
    tw = -(-cols // 32)
    for b in range(COUNT):
        w32 = np.ascontiguousarray(ws[b][:, 2: 2 + cols])
        _e_out, e_w, _worst = tables_int(w32, np.zeros((tw, 32, 32)), "rows")
        emu = bm.tile_error_tables_emulation(w32, np.zeros((tw, 32, 32)))[1]
        assert np.array_equal(emu.view(np.uint64), e_w.view(np.uint64))
        assert np.array_equal(got[b].view(np.uint64), emu.view(np.uint64)), (b, int(np.count_nonzero(got[b] != emu)))


def test_the_wrapper_refuses_what_the_launch_cannot_read():
    torch.cuda.set_device(0)
    x = torch.zeros((2, 64, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.tile_sq_error_batched(x.transpose(1, 2))
    with pytest.raises(hb.MtqError, match="bfloat16 or float32"):
        hb.tile_sq_error_batched(x.double())
    with pytest.raises(hb.MtqError, match="overlap"):
        hb.tile_sq_error_batched(x[0].expand(2, 64, 64))
    with pytest.raises(hb.MtqError, match="at least"):
        hb.tile_sq_error_batched(x, out=torch.empty((2, 3, 4), dtype=torch.float64, device="cuda"))
