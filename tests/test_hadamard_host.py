"""Block Hadamard rotation on the host (quantization_analysis_amd/hadamard.py): the oracle against an explicit Sylvester matrix, the
block rules, and the refusals that need no device."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hadamard as hd
from quantization_analysis_amd import hip_backend as hb


def test_emulation_is_the_product_with_the_sylvester_matrix():
    h = np.array([[1.0]])
    while h.shape[0] < 32:
        h = np.block([[h, h], [h, -h]])
    x = np.random.default_rng(0).standard_normal((3, 96)).astype(np.float32)
    want = ((x.astype(np.float64).reshape(-1, 32) @ h) * np.float64(hd.scale(32))).astype(np.float32).reshape(x.shape)
    assert hd.scale(32) == np.float32(2.0 ** -2.5)
    assert np.array_equal(hd.hadamard_emulation(x, 32).numpy().view(np.uint32), want.view(np.uint32))


def test_twice_is_the_identity_on_small_integers():
    x = torch.from_numpy(np.random.default_rng(1).integers(-8, 9, (5, 192)).astype(np.float32))
    for dtype in (torch.float32, torch.bfloat16):       # even p: a power-of-two scale, every value exact in bf16
        y = hd.hadamard_emulation(hd.hadamard_emulation(x, 64, dtype), 64, dtype)
        assert y.dtype == dtype and torch.equal(y.float(), x)


def test_auto_block():
    assert [hd.auto_block(k) for k in (4096, 7168, 14336, 96)] == [4096, 1024, 2048, 32]
    for k in (16, 48, 1000, 0):
        with pytest.raises(ValueError):
            hd.auto_block(k)


@pytest.mark.parametrize("k, block, kwargs", [
    (96, 48, {}), (64, 16, {}), (8192, 8192, {}), (96, 64, {}),
    (64, 32, {"out_dtype": torch.float32, "q_fmt": "bfp8"}),
])
def test_refusals_need_no_device(k, block, kwargs):
    x = torch.zeros((2, k), dtype=torch.bfloat16)
    if not kwargs:
        with pytest.raises(ValueError):
            hd.check_block(k, block)
    with pytest.raises(hb.MtqError) as e:
        hb.hadamard_rows(x, block, **kwargs)
    assert "device" not in str(e.value)
