"""mtq_hadamard_rows (csrc/mtq_hadamard.hip) on the MI355X against the float64 oracle hadamard_emulation.

Exact regime: integer inputs in [−8, 8] keep every butterfly sum exact in float32 (|S| <= 2^15 at B = 4096), so the contract pins every
output bit, odd p included.  Random regime: the first-order bound of p tree levels plus the scaling multiply, with one unit of slack
for the final rounding, |y − y64| <= (p + 2) · 2^−24 · c_p · Σ|x_i| over the output's block, every element included."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hadamard as hd
from quantization_analysis_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
BLOCKS = [32, 64, 256, 512, 1024, 2048, 4096]
DTYPES = [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)]


def _bits(t: torch.Tensor) -> np.ndarray:
    t = t.cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def _strided(host: torch.Tensor, pad: int = 8, offset: int = 3) -> torch.Tensor:
    """host (rows, k) on the device as a view with row stride k + pad, offset elements into its storage."""
    rows, k = host.shape
    buf = torch.zeros(offset + rows * (k + pad), dtype=host.dtype, device="cuda")
    view = buf[offset:].view(rows, k + pad)[:, :k]
    view.copy_(host)
    return view


@pytest.mark.parametrize("strided", [False, True], ids=["one-block", "three-blocks-strided"])
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=["bf16-bf16", "bf16-f32", "f32-f32"])
@pytest.mark.parametrize("block", BLOCKS)
def test_exact_on_small_integers(block, in_dtype, out_dtype, strided):
    rows, k = (5, 3 * block) if strided else (1, block)
    host = torch.from_numpy(np.random.default_rng(block + rows).integers(-8, 9, (rows, k)).astype(np.float32)).to(in_dtype)
    # base offsets in elements: bf16 in at 16 bytes (vector loads), f32 in at 12 (element loads); likewise the stores
    x = _strided(host, offset=8 if in_dtype == torch.bfloat16 else 3) if strided else host.cuda()
    out = _strided(torch.zeros((rows, k), dtype=out_dtype), pad=16, offset=1 if in_dtype != out_dtype else 8) if strided else None
    y = hb.hadamard_rows(x, block, out=out, out_dtype=out_dtype)
    assert y.dtype == out_dtype and tuple(y.shape) == (rows, k)
    assert np.array_equal(_bits(y), _bits(hd.hadamard_emulation(host, block, out_dtype)))
    assert torch.equal(x.cpu(), host)


def _heavy(rows: int, k: int, block: int) -> np.ndarray:
    x = np.random.default_rng(7).standard_t(3, (rows, k)).astype(np.float32)
    x[1, block: 2 * block] = 0.0
    x[2, 5] = np.float32(2.0 ** 100)
    return x


@pytest.mark.parametrize("block", [32, 1024, 4096])
def test_random_input_within_the_rounding_bound(block):
    p = block.bit_length() - 1
    x = _heavy(3, 2 * block, block)
    y = hb.hadamard_rows(torch.from_numpy(x).cuda(), block).cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64).reshape(-1, block)
    h = np.array([[1.0]])
    while h.shape[0] < block:
        h = np.block([[h, h], [h, -h]])
    c = np.float64(hd.scale(block))
    y64 = ((x64 @ h) * c).reshape(x.shape)
    bound = np.repeat((p + 2) * 2.0 ** -24 * c * np.abs(x64).sum(axis=1), block).reshape(x.shape)
    err = np.abs(y - y64)
    print(f"B={block}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.isfinite(y).all() and (err <= bound).all()
    assert not y[1, block: 2 * block].any()


@pytest.mark.parametrize("block", [32, 1024])
@pytest.mark.parametrize("fmt", ["bfp8", "bfp4", "bfp2"])
def test_quantised_twin_equals_the_row_prepass(fmt, block):
    x = torch.from_numpy(_heavy(3, 3 * block, block)).to(torch.bfloat16).cuda()
    y, yq = hb.hadamard_rows(x, block, q_fmt=fmt)
    assert np.array_equal(_bits(y), _bits(hb.hadamard_rows(x, block)))
    assert np.array_equal(_bits(yq), _bits(hb.quantize_rows_bf16(y, fmt)))
    assert bool((yq != y).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_in_place(dtype):
    block = 256
    x = torch.from_numpy(_heavy(4, 3 * block, block)).to(dtype).cuda()
    want = hb.hadamard_rows(x, block)
    got = hb.hadamard_rows(x, block, out=x)
    assert got is x and np.array_equal(_bits(x), _bits(want))
    with pytest.raises(hb.MtqError):                        # any other overlap is refused
        hb.hadamard_rows(x[:2], block, out=x.view(-1)[block: block + 2 * 3 * block].view(2, 3 * block))
