"""AWQ for BFP on the host: the fixed-exponent oracle against the literal scaled quantiser, the exponent table, a planted salient
channel, and the refusals that need no device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from quantization_analysis_amd import awq, hip_backend as hb
from quantization_analysis_amd.budget_maps import gram_blocks_emulation
from quantization_analysis_amd.gptq import constant_codes
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.quantization_formats import quantize_weight_values


def _weights(kind, n, k, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_t(2, (n, k)) * 0.02).astype(np.float32)
    if kind == "bf16":
        w = torch.from_numpy(w).to(torch.bfloat16).float().numpy()
    w[1, 16:32] = 0.0          # an all-zero group
    w[2, 5] = 0.0              # a lone zero
    return w


@pytest.mark.parametrize("fmt", awq.AWQ_FORMATS)
@pytest.mark.parametrize("kind", ["float32", "bf16"])
def test_oracle_is_the_literal_scaled_quantiser(kind, fmt):
    n, k = 40, 96
    w = _weights(kind, n, k, 3)
    p = np.random.default_rng(4).integers(0, 8, k).astype(np.int32)
    got = awq.quantize_emulation(w, constant_codes(n, k, fmt), p)
    want = np.ldexp(quantize_weight_values(np.ldexp(w, p).astype(np.float32), fmt), -p).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[1, 16:32].any() and not np.signbit(got[1, 16:32]).any() and got[2, 5] == 0.0
    assert np.array_equal(awq.quantize_emulation(w, constant_codes(n, k, "bf16"), p), quantize_weight_values(w, "bf16"))   # bf16 ignores p
    assert np.array_equal(awq.scale_weight(torch.from_numpy(w), p).numpy(), np.ldexp(w, p))


def test_exponent_table():
    rng = np.random.default_rng(0)
    h = np.zeros((3, 32, 32))
    d = rng.uniform(0.5, 200.0, 96) ** 2
    d[[7, 40]] = 0.0                                                    # dead channels
    h[:, np.arange(32), np.arange(32)] = d.reshape(3, 32)
    t = awq.channel_log2(h, 10)
    live = d > 0
    assert np.allclose(t[live], np.log2(np.sqrt(d[live] / 10))) and t[7] == t[40] == t[live].min()
    alphas, p = awq.exponent_table(t[:90], 20, 3)
    assert p.dtype == np.int8 and p.shape[1] == 90 and not p[0].any() and alphas[0] == 0.0 and p.max() == 3
    pad = np.zeros((p.shape[0], 96), dtype=np.int8)
    pad[:, :90] = p
    assert (np.where(np.arange(96) < 90, pad, 99).reshape(-1, 6, 16).min(axis=2) == 0).all()      # every group's minimum is 0
    assert len({r.tobytes() for r in p}) == p.shape[0] < 20 and (np.diff(alphas) > 0).all()       # duplicates dropped, smallest α kept
    assert isinstance(awq.channel_log2(np.zeros((1, 32, 32)), 5), str) and isinstance(awq.channel_log2(h, 0), str)


def test_planted_salient_channel_beats_rtn():
    rng = np.random.default_rng(7)
    n, k, m = 32, 64, 96
    w = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32))
    x = rng.standard_normal((m, k)).astype(np.float32)
    x[:, 9] *= 64.0                                                     # one activation channel 64× its neighbours
    chunk = lambda: [Chunk(x=torch.from_numpy(x).to(torch.bfloat16))]
    h, tokens = gram_blocks_emulation(chunk(), k)
    got = awq.search(chunk(), w, constant_codes(n, k, "bfp4"), h, tokens, "emulation")
    print(got.g, got.alpha, got.losses)
    assert got.g > 0 and got.losses[got.g] < 0.8 * got.losses[0] and got.p_row[9] > 0 and got.losses[0] == got.losses.max()


def test_refusals_without_a_device():
    w = np.ones((4, 16), dtype=np.float32)
    codes = constant_codes(4, 16, "bfp8")
    huge = w.copy()
    huge[0, 0] = np.float32(2.0 ** 120)
    assert "240" in awq.check_weight(huge) and awq.check_weight(w) is None
    assert isinstance(awq.search([], huge, codes, np.eye(32)[None], 4), str)
    with pytest.raises(ValueError):
        awq.exponent_table(np.zeros(16), 20, 8)
    with pytest.raises(ValueError):
        awq.quantize_emulation(w, codes, np.full(16, 9))
    with pytest.raises(ValueError):
        awq.scale_weight(np.full((1, 16), 3e38, dtype=np.float32), np.full(16, 7))
    L = hb.lib()
    assert L.mtq_awq_losses_scratch_doubles(129, 65, 20) == 2 * 2 * 5 and hb.awq_slots() == 5 and L.mtq_awq_losses_scratch_doubles(0, 5, 1) == 0
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)
    ok = dict(x=ptr, m=4, k=16, ldx=16, w=ptr, w_dtype=hb.DTYPE_F32, n=4, ldw=16, codes=ptr, code_count=1, p=ptr, g_count=1, loss=ptr,
              scratch=ptr, scratch_doubles=64, stream=None)
    for bad in (dict(x=None), dict(w_dtype=7), dict(m=0), dict(g_count=0), dict(ldx=15), dict(ldw=8), dict(code_count=2), dict(scratch_doubles=1)):
        assert L.mtq_awq_losses(*{**ok, **bad}.values()) == -1, bad
    okq = dict(w=ptr, w_dtype=hb.DTYPE_BF16, n=4, k=16, ldw=16, codes=ptr, code_count=1, p_row=ptr, out=ptr, ldo=16, stream=None)
    for bad in (dict(out=None), dict(w_dtype=-1), dict(k=0), dict(ldo=15), dict(code_count=0)):
        assert L.mtq_awq_quantize(*{**okq, **bad}.values()) == -1, bad
