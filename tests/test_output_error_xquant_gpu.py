"""Layer-output error with BFP-quantised activations on the MI355X (csrc/mtq_output_error.hip: the row pre-pass
mtq_quantize_rows_bf16 and the QX launch mtq_output_error_qx).

  * the pre-pass writes the upper halves of K2's float32 y (mtq_quantize) for every bf16 input, specials included, and on finite
    groups the host quantize_weight_values;
  * the QX sums against the float64 emulation within the f32-accumulation bound, with Q(X) in place of X on the candidate side;
  * exact probes: X on an integer grid that Q(X) rounds, and one-hot W, where every output is exact, so the sums
    may differ from the emulation's only by the float64 summation order; a one-step mutation of the oracle's Q(X) must show;
  * xq = x gives the sums of mtq_output_error bit for bit; determinism, chunking and the CLI."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import SLOTS, emulation_sums, hip_sums
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.inputs import gen
from tests.test_output_error_exact_gpu import GRID, bounds, grid_operands, map_image, verdict
from tests.test_output_error_gpu import SHAPES, _check, _eps
from tests.test_output_error_host import make_fixture

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FMTS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
XF = ["bfp8", "bfp4", "bfp2"]


def _bf16(bits_u16: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits_u16, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _k2_upper(xd: torch.Tensor, fmt: str) -> np.ndarray:
    y = hb.quantize(xd, fmt).cpu().numpy().view(np.uint32)
    assert not (y & 0xFFFF).any(), "a BFP / bf16 value with nonzero low 16 bits"
    return (y >> 16).astype(np.uint16)


def _special_population(seed: int = 0) -> np.ndarray:
    """bf16 bit patterns, 32 per row: every pattern in order and shuffled (binades, ±0, subnormals, ±Inf, NaNs, in uniform and in
    mixed groups), then groups built around a chosen shared exponent — the fast-route borders 79 / 80 / 180 / 181, the literal ranges
    and the specials — whose other elements lie 0..40 binades lower, with mantissas biased to BFP ties and to the saturating top."""
    rng = np.random.default_rng(seed)
    every = np.arange(1 << 16, dtype=np.uint16)
    parts = [every.reshape(-1, 32), rng.permutation(every).reshape(-1, 32)]
    groups = []
    for E in [79, 80, 180, 181, 1, 2, 24, 25, 127, 230, 231, 254, 0, 255]:
        for _ in range(64):
            e = np.clip(E - rng.integers(0, 41, 16), 0, 255)
            e[rng.integers(0, 16)] = E
            mant = rng.integers(0, 128, 16)
            tie = rng.random(16) < 0.4                       # ...1000 patterns: a tie of bfp2 / bfp4 / bfp8
            mant[tie] = (rng.integers(0, 8, tie.sum()) << 4) | 0x8 if E % 2 else (rng.integers(0, 64, tie.sum()) << 1) | 1
            top = rng.random(16) < 0.15                      # 1.1111111: rounds up past the largest code
            mant[top] = 0x7F
            sign = rng.integers(0, 2, 16) << 15
            groups.append((sign | (e << 7) | mant).astype(np.uint16))
    parts.append(np.concatenate(groups).reshape(-1, 32))
    return np.concatenate(parts)


@pytest.mark.parametrize("fmt", ["bf16", "bfp8", "bfp4", "bfp2"])
def test_prepass_bits_equal_k2_upper_halves(fmt):
    torch.cuda.set_device(0)
    pat = _special_population()
    xd = _bf16(pat).cuda()
    got = _bits(hb.quantize_rows_bf16(xd, fmt))
    want = _k2_upper(xd, fmt)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(tuple(i), hex(pat[tuple(i)]), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:8]]
    if fmt == "bf16":
        assert np.array_equal(got, pat)
    # the finite groups against the host oracle (a group holding Inf / NaN is left out; its bits were pinned to K2 above)
    x32 = (pat.astype(np.uint32) << 16).view(np.float32)
    finite = np.repeat(np.isfinite(x32.reshape(-1, 16)).all(axis=1), 16).reshape(x32.shape)
    host = quantize_weight_values(np.where(finite, x32, 0.0).astype(np.float32), fmt).view(np.uint32)
    assert not (host[finite] & 0xFFFF).any()
    assert np.array_equal(got[finite], (host[finite] >> 16).astype(np.uint16))


@pytest.mark.parametrize("k", [1, 15, 16, 17, 33, 7171])
@pytest.mark.parametrize("fmt", XF)
def test_prepass_ragged_and_strided(k, fmt):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(k)
    m = 37
    wide = (rng.standard_normal((m, k + 5)) * np.exp2(rng.integers(-20, 20, (m, 1)))).astype(np.float32)
    xw = torch.from_numpy(wide).to(torch.bfloat16).cuda()
    for xd in (xw[:, :k].contiguous(), xw[:, 3: k + 3]):      # contiguous, and strided with an odd offset
        got = _bits(hb.quantize_rows_bf16(xd, fmt))
        assert np.array_equal(got, _k2_upper(xd, fmt))
        assert np.array_equal(got, (quantize_weight_values(xd.float().cpu().numpy(), fmt).view(np.uint32) >> 16).astype(np.uint16))
    out = torch.full((m, k + 9), -1.0, dtype=torch.bfloat16, device="cuda")    # a strided destination: the pads stay as they were
    hb.quantize_rows_bf16(xw[:, 3: k + 3], fmt, out=out[:, 2: k + 2])
    o = out.cpu()
    assert np.array_equal(_bits(o[:, 2: k + 2]), _k2_upper(xw[:, 3: k + 3], fmt))
    assert bool((o[:, :2] == -1).all()) and bool((o[:, k + 2:] == -1).all())


# ----------------------------------------------------------------------------- the QX launch against the emulation


def _operands(m, n, k, kind, with_bias, seed):
    w = gen(kind, seed, (n, k))
    x = torch.from_numpy(gen("normal_bf16", seed + 1, (m, k)) * 40).to(torch.bfloat16)
    bias = gen("normal_f32", seed + 2, (n,)) if with_bias else None
    wt = torch.from_numpy(w).to(torch.bfloat16 if kind.endswith("bf16") else torch.float32)
    return x, wt, bias


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("kind", ["heavy_bf16", "heavy_f32", "normal_f32"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("x_format", XF)
def test_qx_sums_match_emulation(m, n, k, kind, with_bias, x_format):
    torch.cuda.set_device(0)
    seed = m * 7 + n * 13 + k
    x, wt, bias = _operands(m, n, k, kind, with_bias, seed)
    rec = (x.float() @ wt.float().T + (0 if bias is None else torch.from_numpy(bias))).to(torch.bfloat16)
    bt = None if bias is None else torch.from_numpy(bias)
    wf = wt.float().numpy()
    amap = np.random.default_rng(seed).integers(0, 4, size=(-(-n // 32), -(-k // 32))).astype(np.int8)
    my = map_image(wf, amap)
    want, mm, seen, _ = emulation_sums([Chunk(x=x, recorded=rec)], wt, FMTS, bt, my, x_format=x_format)
    got, mg, seen_g, _ = hip_sums([Chunk(x=x, recorded=rec)], wt, FMTS, bt, amap, x_format=x_format)
    assert mm == mg == m and seen and seen_g
    count = float(m * n)
    xf = x.float().numpy()
    qx = quantize_weight_values(xf, x_format)
    eps_r = _eps(xf, [wf], bias, k)
    for f in FMTS:
        eps_q = 0.0 if f == "fp0" else _eps(qx, [quantize_weight_values(wf, f)], bias, k)
        _check(got[SLOTS.index(f)], want[SLOTS.index(f)], count, eps_r, eps_q, f)
    _check(got[SLOTS.index("map")], want[SLOTS.index("map")], count, eps_r, _eps(qx, [my], bias, k), "map")
    _check(got[SLOTS.index("recorded")], want[SLOTS.index("recorded")], count, eps_r, 0.0, "recorded")
    # fp0 and recorded do not see Q(X): the same bits as the launch without it
    plain, *_ = hip_sums([Chunk(x=x, recorded=rec)], wt, FMTS, bt, amap)
    for s in ("fp0", "recorded"):
        assert np.array_equal(got[SLOTS.index(s)].view(np.uint64), plain[SLOTS.index(s)].view(np.uint64)), s


@pytest.mark.parametrize("kind", ["heavy_bf16", "heavy_f32"])
def test_xq_equal_to_x_is_bit_identical_to_the_plain_launch(kind):
    torch.cuda.set_device(0)
    m, n, k = 300, 130, 70
    x, wt, bias = _operands(m, n, k, kind, True, 5)
    xd, wd, bd = x.cuda(), wt.cuda(), torch.from_numpy(bias).cuda()
    rec = (x.float() @ wt.float().T).cuda()
    ad = torch.from_numpy(np.random.default_rng(1).integers(0, 4, size=(5, 3)).astype(np.int8)).cuda()
    a = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    c = torch.zeros_like(a)
    hb.output_error(xd, wd, 0xF, a, bias=bd, assignment=ad, recorded=rec)
    hb.output_error(xd, wd, 0xF, b, bias=bd, assignment=ad, recorded=rec, xq=xd)
    hb.output_error(xd, wd, 0xF, c, bias=bd, assignment=ad, recorded=rec, xq=hb.quantize_rows_bf16(xd, "bf16"))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))


def test_qx_deterministic_and_chunked():
    torch.cuda.set_device(0)
    n, k, m = 130, 70, 1000
    w = torch.from_numpy(gen("heavy_f32", 21, (n, k)))
    bias = torch.from_numpy(gen("normal_f32", 22, (n,)))
    x = torch.from_numpy(gen("normal_bf16", 23, (m, k)) * 20).to(torch.bfloat16)
    one, *_ = hip_sums([Chunk(x=x)], w, FMTS, bias, x_format="bfp4")
    two, *_ = hip_sums([Chunk(x=x)], w, FMTS, bias, x_format="bfp4")
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    parts, *_ = hip_sums([Chunk(x=x[s: s + 130]) for s in range(0, m, 130)], w, FMTS, bias, x_format="bfp4")
    for f in FMTS:   # Q(X) is row-local and every output is formed as in one chunk: only the float64 summation order differs
        _check(parts[SLOTS.index(f)], one[SLOTS.index(f)], float(m * n), 0.0, 0.0, f)


# ----------------------------------------------------------------------------- exact probes


def _expect(x, qx, w, bias, images: dict, unit):
    """slot → bounds() from the exact per-output values: R from X, every candidate from Q(X), fp0 from the bias."""
    b = 0.0 if bias is None else np.asarray(bias, np.float64)
    r = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + b
    out = {SLOTS.index(f): bounds(r, np.asarray(qx, np.float64) @ np.asarray(images[f], np.float64).T + b, unit=unit) for f in images}
    out[SLOTS.index("fp0")] = bounds(r, np.broadcast_to(b, r.shape), unit=unit)
    return out


def _run(x, w, bias, x_format, amap=None):
    got, *_ = hip_sums([Chunk(x=torch.from_numpy(x).to(torch.bfloat16))], torch.from_numpy(w), ["bf16", "bfp8", "bfp4", "bfp2"],
                       None if bias is None else torch.from_numpy(bias), amap, x_format=x_format)
    return got


@pytest.mark.parametrize("m,n,k", [(37, 50, 40), (200, 130, 192), (129, 64, 33)])
@pytest.mark.parametrize("x_format", XF)
@pytest.mark.parametrize("with_bias", [False, True])
def test_exact_integer_grid(m, n, k, x_format, with_bias):
    """X integers in [-255, 255] (8 significant bits: Q(X) rounds them), W and the bias on the 2⁻⁸ grid.  Q(X) holds integers of
    at most 256, so with K·255·max Σ|w| below 2²⁴ grid units every f32 partial sum is exact."""
    torch.cuda.set_device(0)
    _x, w, bias = grid_operands(m, n, k, m + n + k, with_bias)
    rng = np.random.default_rng(k)
    x = (rng.integers(-255, 256, size=(m, k)) >> rng.integers(0, 6, size=(m, -(-k // 16))).repeat(16, axis=1)[:, :k]).astype(np.float32)
    qx = quantize_weight_values(x, x_format)
    images = {f: quantize_weight_values(w, f) for f in ["bf16", "bfp8", "bfp4", "bfp2"]}
    assert not np.array_equal(qx, x), "Q(X) must round somewhere"
    assert np.array_equal(qx, np.round(qx)) and np.abs(qx).max() <= 256 and np.abs(x).max() <= 255
    b = np.zeros(1) if bias is None else bias
    for v in [w, *images.values(), b]:
        assert np.array_equal(v / GRID, np.round(v / GRID)) and np.abs(v).max(initial=0) <= 1.0
    worst = 256 * max(np.abs(v.astype(np.float64)).sum(axis=1).max() for v in [w, *images.values()]) + np.abs(b).max()
    assert worst / GRID < 2.0 ** 24
    got = _run(x, w, bias, x_format)
    assert verdict(got, emulation_sums([Chunk(x=torch.from_numpy(x).to(torch.bfloat16))], w, ["bf16", "bfp8", "bfp4", "bfp2"], bias,
                                       x_format=x_format)[0], _expect(x, qx, w, bias, images, GRID)) == []


def _one_hot(n, k, seed):
    rng = np.random.default_rng(seed)
    w = np.zeros((n, k), np.float32)
    w[np.arange(n), np.arange(n) % k] = np.exp2(rng.integers(-4, 5, n)) * rng.choice([-1, 1], n)
    return w


@pytest.mark.parametrize("m,n,k", [(70, 96, 48), (129, 66, 33), (64, 256, 200)])
@pytest.mark.parametrize("x_format", XF)
def test_exact_one_hot_w_pins_the_quantiser(m, n, k, x_format):
    """Each row of W a single ±2ˢ at column n mod K, so output (m, n) is 2ˢ·Q(X)[m, n mod K] for every candidate (the BFP image of a
    lone power of two is itself) and every element of Q(X) appears in some output.  X normal bf16 over ±40 binades (no subnormal
    product), groups mixing magnitudes so that Q(X) drops and rounds elements.  A one-step change of one element of the oracle's
    Q(X) must make the comparison fail."""
    torch.cuda.set_device(0)
    rng = np.random.default_rng(m + k)
    x = (rng.standard_normal((m, k)) * np.exp2(rng.integers(-40, 40, (m, k)) // 8 * 8)).astype(np.float32)
    x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.all(np.abs(x[x != 0]) >= 2.0 ** -100)
    w = _one_hot(n, k, k)
    qx = quantize_weight_values(x, x_format)
    assert not np.array_equal(qx, x)
    images = {f: quantize_weight_values(w, f) for f in ["bf16", "bfp8", "bfp4", "bfp2"]}
    for v in images.values():
        assert np.array_equal(v, w)
    got = _run(x, w, None, x_format)
    assert verdict(got, _want_from(x, qx, w, images), _expect(x, qx, w, None, images, None)) == []
    # the probe can fail: one element of Q(X), moved by one BFP step of its group
    i, j = map(int, np.argwhere(qx != 0)[0])
    step = np.float32(2.0 ** (np.floor(np.log2(np.abs(x[i, (j // 16) * 16: (j // 16) * 16 + 16]).max())) - {"bfp8": 6, "bfp4": 2, "bfp2": 0}[x_format]))
    bad = qx.copy()
    bad[i, j] = bad[i, j] - np.sign(bad[i, j]) * step
    assert verdict(got, _want_from(x, bad, w, images), _expect(x, bad, w, None, images, None)) != []


def _want_from(x, qx, w, images):
    """float64 sums from given Q(X) (the oracle's, or a mutation of it) in the emulation's order."""
    r = torch.from_numpy(np.asarray(x, np.float64)) @ torch.from_numpy(np.asarray(w, np.float64)).T
    from quantization_analysis_amd.output_error import _fold64

    sums = np.zeros((len(SLOTS), 7))
    q64 = torch.from_numpy(np.asarray(qx, np.float64))
    for f, img in images.items():
        _fold64(sums[SLOTS.index(f)], r, q64 @ torch.from_numpy(np.asarray(img, np.float64)).T)
    _fold64(sums[SLOTS.index("fp0")], r, torch.zeros_like(r))
    return sums


def test_cli_hip_agrees_with_emulation_with_x_format(tmp_path):
    model, io = make_fixture(tmp_path)
    docs = {}
    for backend in ("emulation", "hip"):
        out = tmp_path / backend
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0.mlp",
                            "--backend", backend, "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--compression-config",
                            str(ROOT / "compression_configs" / "greedy_seed123.json"), "--x-format", "bfp8", "--out-dir", str(out)],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "X bfp8" in r.stdout
        docs[backend] = json.loads((out / "layer_output_error.json").read_text())
        assert docs[backend]["x_format"] == "bfp8"
    for oe, oh in zip(docs["emulation"]["ops"], docs["hip"]["ops"]):
        assert oe["op"] == oh["op"] and oe["M"] == oh["M"]
        for re_, rh in zip(oe["rows"], oh["rows"]):
            assert re_["candidate"] == rh["candidate"] and re_["bytes"] == rh["bytes"]
            assert abs(re_["pcc"] - rh["pcc"]) < 1e-5, (oe["op"], re_, rh)
            for key in ("mae", "atol"):
                assert abs(re_[key] - rh[key]) <= 1e-5 * max(1.0, abs(re_[key])), (oe["op"], re_, rh)
