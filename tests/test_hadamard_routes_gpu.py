"""The block Hadamard rotation through its two routes on the MI355X: evaluate_op(rotate=B) on hip against the emulation, and
PackedLinear / PackedMatmul(rotate=B) against the unrotated float64 product.

LOE: small-integer W and X at B = 64 (even p: a power-of-two scale) make W′ and X′ bit-equal on both backends, so the rows differ only by
the fused kernel's float32 accumulation: the bounds restated from test_output_error_gpu.py (mae / atol within ε_r + ε_q, pcc within
2ε_r/σ_r + 2ε_q/σ_q, ε = (k + 2)·2⁻²⁴·(1 + 2⁻⁷)·max Σ|x·w|) and, for the GPTQ rows, test_gptq_gpu.py's 5 % on the calibration loss and
on the held-out SSE.  Packed: x in {−1, 0, 1} and integer W in [−2, 2] make X′ and W′ multiples of 1/8 below 16, exact in bf16, and
every product and partial sum exact in float32: the rotation is invisible, bit for bit."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hadamard as hd
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from quantization_analysis_amd.layer_io import OpIO
from quantization_analysis_amd.output_error import SLOTS, evaluate_op
from quantization_analysis_amd.quantization_formats import quantize_weight_values

pytestmark = pytest.mark.gpu
N, K, M, B = 64, 128, 96, 64
FMTS = ["bf16", "bfp8", "bfp4"]


class _Index:
    """The two calls evaluate_op makes on a model index, over one in-memory weight."""

    def __init__(self, w):
        self.w = w

    def shape_dtype(self, name):
        return tuple(self.w.shape), self.w.dtype

    def load(self, name, device=None):
        return self.w if device is None else self.w.to(device)


@pytest.fixture(scope="module")
def op_case(tmp_path_factory):
    rng = np.random.default_rng(11)
    w = torch.from_numpy(rng.integers(-4, 5, (N, K)).astype(np.float32))
    root, samples, xs = tmp_path_factory.mktemp("rotated_op"), [], {}
    for idx, split in enumerate(("calibration", "test")):
        x = torch.from_numpy(rng.integers(-3, 4, (M if split == "test" else 2 * K, K)).astype(np.float32)).to(torch.bfloat16)
        path = root / f"sample_{idx}.pt"
        torch.save({"args": (x,), "kwargs": {}, "output": (x.float() @ w.T).to(torch.bfloat16)}, path)
        samples.append((split, idx, path))
        xs[split] = x
    ops = {s: OpIO(op="op", weight="op.weight", bias=None, samples=[t for t in samples if t[0] == s]) for s in xs}
    return _Index(w), ops, w, xs["test"]


def _eps(xa, wa):
    return (K + 2) * 2.0 ** -24 * (1 + 2.0 ** -7) * float((np.abs(xa) @ np.abs(wa).T).max())


def _check(got, want, count, eps_r, eps_q, what):
    g, e = hb.columns_from_sums(np.asarray(got), count), hb.columns_from_sums(np.asarray(want), count)
    print(what, "hip", g["pcc"], g["mae"], g["atol"], "emulation", e["pcc"], e["mae"], e["atol"])
    f64 = 64 * count * 2.0 ** -53
    assert abs(g["mae"] - e["mae"]) <= eps_r + eps_q + f64 * abs(e["mae"]) + 1e-300, what
    assert abs(g["atol"] - e["atol"]) <= eps_r + eps_q + 2.0 ** -52 * abs(e["atol"]) + 1e-300, what
    mr, mq = want[0] / count, want[2] / count
    sr, sq = np.sqrt(max(want[1] / count - mr * mr, 0.0)), np.sqrt(max(want[3] / count - mq * mq, 0.0))
    rms = np.sqrt(want[1] / count) * np.sqrt(max(want[3] / count, 0.0))
    assert sr > 0.0 and sq > 0.0
    assert abs(g["pcc"] - e["pcc"]) <= 2 * eps_r / sr + 2 * eps_q / sq + f64 * rms / (sr * sq), what


@pytest.mark.parametrize("x_format", ["bf16", "bfp8"])
def test_rotated_rows_on_hip_match_the_emulation(op_case, x_format):
    torch.cuda.set_device(0)
    index, ops, w, x = op_case
    rh = evaluate_op(index, ops["test"], FMTS, None, "hip", x_format=x_format, rotate=B)
    re_ = evaluate_op(index, ops["test"], FMTS, None, "emulation", x_format=x_format, rotate=B)
    assert rh.rotate == re_.rotate == B and rh.skipped is None and rh.m == re_.m == M
    assert [r.candidate for r in rh.rows] == [r.candidate for r in re_.rows] == FMTS + ["recorded"]
    wr = hd.rotate_weight(w, B).numpy()
    xr = hd.hadamard_emulation(x, B, torch.bfloat16)
    assert torch.equal(hd.hadamard(x, B, backend="hip").cpu(), xr) and torch.equal(hd.rotate_weight(w, B, backend="hip").cpu(), torch.from_numpy(wr))
    xq = xr.float().numpy() if x_format == "bf16" else quantize_weight_values(xr.float().numpy(), x_format)
    eps_r = _eps(xr.float().numpy(), wr)
    for a, b in zip(rh.rows, re_.rows):
        eps_q = 0.0 if a.candidate == "recorded" else _eps(xq, quantize_weight_values(wr, a.candidate))
        _check(a.sums, b.sums, float(M * N), eps_r, eps_q, f"{x_format} {a.candidate}")
    # the rotated layer is the layer: its R against the recorded X·Wᵀ differs only by the recorded output's bf16 rounding
    assert rh.rows[-1].pcc > 0.9999


def test_rotated_gptq_rows_and_unrotated_rows(op_case):
    torch.cuda.set_device(0)
    index, ops, _w, _x = op_case
    rh = evaluate_op(index, ops["test"], FMTS, None, "hip", calib=ops["calibration"], gptq=True, rotate=B)
    re_ = evaluate_op(index, ops["test"], FMTS, None, "emulation", calib=ops["calibration"], gptq=True, rotate=B)
    assert [r.candidate for r in rh.rows][-2:] == [r.candidate for r in re_.rows][-2:] == ["gptq:bfp8", "gptq:bfp4"] and rh.budget_skipped == []
    sse = lambda s: float(s[1] - 2.0 * s[4] + s[3])
    for a, b in zip(rh.rows[-2:], re_.rows[-2:]):
        print(a.candidate, a.extra["calib_loss"], b.extra["calib_loss"], sse(a.sums), sse(b.sums))
        assert a.extra["calib_tokens"] == b.extra["calib_tokens"] == 2 * K
        assert abs(a.extra["calib_loss"] - b.extra["calib_loss"]) <= 0.05 * b.extra["calib_loss"] + 1e-12
        assert abs(sse(a.sums) - sse(b.sums)) <= 0.05 * sse(b.sums) + 1e-12
    plain, zero = evaluate_op(index, ops["test"], FMTS, None, "hip"), evaluate_op(index, ops["test"], FMTS, None, "hip", rotate=0)
    assert zero.rotate == 0 and [(r.candidate, r.sums) for r in zero.rows] == [(r.candidate, r.sums) for r in plain.rows]
    assert evaluate_op(index, ops["test"], FMTS, None, "hip", rotate=256).skipped    # 256 does not divide k = 128


@pytest.mark.parametrize("m, kernel", [(4, "skinny"), (96, "block")])
@pytest.mark.parametrize("kn", [False, True], ids=["PackedLinear", "PackedMatmul"])
def test_rotation_is_invisible_in_exact_arithmetic(kn, m, kernel):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(m + kn)
    x = torch.from_numpy(rng.integers(-1, 2, (m, K)).astype(np.float32))
    w = torch.from_numpy(rng.integers(-2, 3, (N, K)).astype(np.float32))
    want = (x.double() @ w.double().T).float()
    stored = w.T.contiguous() if kn else w                                     # (k, n) for PackedMatmul: k is axis 0
    rotated = hd.rotate_weight(stored.cuda(), B, axis=0 if kn else -1, backend="hip")
    assert torch.equal(rotated.to(torch.bfloat16).float(), rotated) and not torch.equal(rotated.cpu(), stored)
    amap = np.zeros((-(-rotated.shape[0] // 32), -(-rotated.shape[1] // 32)), dtype=np.int8)      # every tile bf16
    pt = packed.pack(rotated, amap, backend="hip")
    mod = (packed.PackedMatmul if kn else packed.PackedLinear)(pt, kernel=kernel, rotate=B)
    assert torch.equal(mod(x.to(torch.bfloat16).cuda()).cpu(), want)
    with pytest.raises(ValueError):
        (packed.PackedMatmul if kn else packed.PackedLinear)(pt, rotate=48)
