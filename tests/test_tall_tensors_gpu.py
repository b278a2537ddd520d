"""Tensors taller than one launch's grid: the row-looping kernels launch min(rows, 65535) blocks in y (K2T / K3T: min(row groups,
65535), 16 rows a group) and stride over the rest, so only a tensor past that limit runs their loops a second and a third time.  Real
ones do: 128256 × 4096 embeddings and heads, 129280 × 7168.  Each kernel is compared with the oracle or the emulation bit for bit at a
row count that is no multiple of 65535 (the last pass is partial), y written into a sentinel-filled buffer with ldy > cols and rows
to spare, which must stay untouched: a pass that skips rows, or writes past them, shows."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import quantization_formats as qf
from tests.inputs import gen, to_bf16_valued

pytestmark = pytest.mark.gpu

GRID_Y = 65535
TALL = 131101                 # two full passes of 65535 rows and a partial third
TALL_T = 1048613              # 65538 row groups of 16 and a partial 65539th: past 65535 row groups
SENTINEL = 0x7FBADBAD         # a NaN no kernel writes
SPARE_ROWS = 3
STORAGE = {"bf16": torch.bfloat16, "f32": torch.float32}
MIXED = ["bf16", "bfp8", "bfp4", "bfp2"]


def host_x(storage: str, rows: int, cols: int, seed: int) -> np.ndarray:
    x = gen("heavy_f32", seed, (rows, cols))
    return to_bf16_valued(x) if storage == "bf16" else x


def device_view(x: np.ndarray, storage: str, ld: int):
    """x as a (rows, cols) view with leading dimension ld of a device buffer in the storage type (exact: bf16 storage gets bf16 values)."""
    rows, cols = x.shape
    wide = np.zeros((rows, ld), np.float32)
    wide[:, :cols] = x
    return torch.from_numpy(wide).cuda().to(STORAGE[storage])[:, :cols]


def sentinel_out(rows: int, ldy: int):
    return torch.full((rows + SPARE_ROWS, ldy), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def check_out(y, want: np.ndarray, what) -> None:
    """y[:rows, :cols] has the bits of want; the padding columns and the spare rows keep the sentinel."""
    rows, cols = want.shape
    got = y.cpu().numpy().view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(got[:rows, :cols] != w)
    assert bad.size == 0, (what, "rows", np.unique(bad[:, 0])[:8], "of", len(np.unique(bad[:, 0])))
    assert (got[:rows, cols:] == SENTINEL).all(), (what, "padding columns written")
    assert (got[rows:] == SENTINEL).all(), (what, "rows past the tensor written")


def aligned16(t) -> bool:
    return t.data_ptr() % 16 == 0


def quad_route(x, y) -> bool:
    """launch_quantize's coalesced quad form (quantize_quads): 16-byte aligned rows of x and y, cols % 16 == 0."""
    _code, _n, _s, _rows, cols, ld = hb._matrix(x, (2,))
    return aligned16(x) and (ld * x.element_size()) % 16 == 0 and aligned16(y) and (y.stride(0) * 4) % 16 == 0 and cols % 16 == 0


def c_quantize(x, code: int, y) -> None:
    dt, _n, _s, rows, cols, ld = hb._matrix(x, (2,))
    hb.check(hb.lib().mtq_quantize(x.data_ptr(), dt, rows, cols, ld, code, y.data_ptr(), y.stride(0), hb._stream_ptr()))


ROUTES = {"quads": (32, 32, 36), "groups": (40, 40, 43)}   # cols, ld, ldy


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("route", list(ROUTES))
def test_k2_quantize_past_the_grid(storage, route):
    cols, ld, ldy = ROUTES[route]
    x = host_x(storage, TALL, cols, 2)
    xd = device_view(x, storage, ld)
    for fmt in ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]:
        y = sentinel_out(TALL, ldy)
        assert quad_route(xd, y) == (route == "quads")
        c_quantize(xd, hb.FMT_CODE[fmt], y)
        check_out(y, orc.quantize_np(x, fmt), (storage, route, fmt))


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("route", list(ROUTES))
def test_k3_apply_assignment_past_the_grid(storage, route):
    cols, ld, ldy = {"quads": (64, 64, 68), "groups": (70, 70, 75)}[route]   # three tile columns
    x = host_x(storage, TALL, cols, 3)
    xd = device_view(x, storage, ld)
    amap = np.random.default_rng(3).integers(0, len(MIXED), size=hb.tiles_hw(TALL, cols), dtype=np.int8)
    mdev = torch.from_numpy(amap).cuda()
    y = sentinel_out(TALL, ldy)
    assert quad_route(xd, y) == (route == "quads")
    dt, _n, _s, rows, _c, ldx = hb._matrix(xd, (2,))
    hb.check(hb.lib().mtq_apply_assignment(xd.data_ptr(), dt, rows, cols, ldx, mdev.data_ptr(), y.data_ptr(), y.stride(0), hb._stream_ptr()))
    check_out(y, orc.apply_assignment(x, amap), (storage, route))


@pytest.mark.parametrize("storage", list(STORAGE))
def test_fp4_proxy_quantize_past_the_grid(storage):
    cols, ldy = 24, 27
    x = host_x(storage, TALL, cols, 5)
    xd = device_view(x, storage, cols)
    for fmt in hb.PROXY_FORMATS:
        y = sentinel_out(TALL, ldy)
        c_quantize(xd, hb.QUANTIZE_CODE[fmt], y)
        check_out(y, qf.quantize_weight_values(x, fmt), (storage, fmt))


K5_CASES = {   # cols, ldw, ldo, scale grid, (bh, bw)
    "blocks128": (256, 256, 260, (1025, 2), (128, 128)),
    "blocks101x84": (250, 252, 256, (1311, 3), (101, 84)),   # no power-of-two block width, a ragged row end
}


@pytest.mark.parametrize("case", list(K5_CASES))
def test_k5_dequant_fp8_past_the_grid(case):
    cols, ldw, ldo, (srows, scols), (bh, bw) = K5_CASES[case]
    rows = TALL
    assert (-(-rows // srows), -(-cols // scols)) == (bh, bw)
    rng = np.random.default_rng(9)
    codes = np.setdiff1d(np.arange(256), [0x7F, 0xFF]).astype(np.uint8)   # no NaN code: every output has one right answer
    w = rng.choice(codes, size=(rows, ldw))
    sc = (np.exp2(rng.integers(-12, 6, size=(srows, scols))) * rng.uniform(1, 2, size=(srows, scols))).astype(np.float32)
    wd = torch.from_numpy(w).cuda()
    scd = torch.from_numpy(sc).cuda()
    out = sentinel_out(rows, ldo)
    assert wd.data_ptr() % 4 == 0 and ldw % 4 == 0 and aligned16(out) and ldo % 4 == 0      # K5's quad form (dequant_fp8_quads)
    hb.check(hb.lib().mtq_dequant_fp8_block(wd.data_ptr(), scd.data_ptr(), rows, cols, ldw, srows, scols, out.data_ptr(), ldo, hb._stream_ptr()))
    check_out(out, orc.dequant_fp8_block(w[:, :cols], sc), case)


@pytest.mark.parametrize("storage", list(STORAGE))
def test_k2t_quantize_transposed_past_the_grid(storage):
    rows, cols, ldy = TALL_T, 5, 7
    assert -(-rows // 16) > GRID_Y and rows % 16
    x = host_x(storage, rows, cols, 11)
    xd = device_view(x, storage, cols)
    xt = np.ascontiguousarray(x.T)
    fn = hb._entry("mtq_quantize_transposed")
    for fmt in ["bf16", "bfp8", "bfp4", "bfp2"]:
        y = sentinel_out(rows, ldy)
        hb.check(fn(xd.data_ptr(), hb._matrix(xd, (2,))[0], rows, cols, cols, hb.FMT_CODE[fmt], y.data_ptr(), ldy, hb._stream_ptr()))
        check_out(y, orc.quantize_np(xt, fmt).T, (storage, fmt))


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("route", ["quad", "scalar"])
def test_k3t_apply_assignment_transposed_past_the_grid(storage, route):
    rows = TALL_T
    cols, ldy = (8, 12) if route == "quad" else (7, 9)
    assert -(-rows // 16) > GRID_Y
    x = host_x(storage, rows, cols, 13)
    xd = device_view(x, storage, cols)
    amap = np.random.default_rng(13).integers(0, len(MIXED), size=hb.tiles_hw(cols, rows), dtype=np.int8)   # Xᵀ's grid
    mdev = torch.from_numpy(amap).cuda()
    y = sentinel_out(rows, ldy)
    esz = xd.element_size()
    quad = cols % 4 == 0 and xd.data_ptr() % (4 * esz) == 0 and aligned16(y) and ldy % 4 == 0
    assert quad == (route == "quad")
    fn = hb._entry("mtq_apply_assignment_transposed")
    hb.check(fn(xd.data_ptr(), hb._matrix(xd, (2,))[0], 1, rows * cols, rows, cols, cols, mdev.data_ptr(), y.data_ptr(), ldy, hb._stream_ptr()))
    check_out(y, orc.apply_assignment(np.ascontiguousarray(x.T), amap).T, (storage, route))
