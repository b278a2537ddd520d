"""GPU parity tests: every HIP kernel, called through the C ABI (libmtq_hip.so), against the CPU oracle
on the same seeded inputs and against the committed golden vectors.  Bit-exact bar for y bits, stats
records (float64, identical summation order) and assignment maps."""
import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb
from tests.inputs import gen

pytestmark = pytest.mark.gpu
ALL = ["bf16", "bfp8", "bfp4", "bfp2"]


def dev(x: np.ndarray, bf16: bool = False):
    """Upload x; bf16=True converts ON THE HOST first (the device cast canonicalises NaN signs/payloads)."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(torch.bfloat16).cuda() if bf16 else t.cuda()


def bits(t) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


def test_native_library_is_loaded():
    hb.require_gpu()
    assert hb.LIB_PATH.exists()
    maps = open("/proc/self/maps").read()
    assert "libmtq_hip.so" in maps


def test_quantize_known_answer_bits(golden_dir):
    d = np.load(golden_dir / "f1_quantize_kat.npz")
    x = d["x_bits"].view(np.float32)
    for fmt in ALL + ["fp0"]:
        y = hb.quantize(dev(x), fmt)
        assert np.array_equal(bits(y), d[f"y_{fmt}"]), fmt


def test_quantize_layouts(golden_dir):
    d = np.load(golden_dir / "f2_layouts.npz")
    names = sorted({k[:-2] for k in d.files if k.endswith("_x")})
    for name in names:
        x = d[f"{name}_x"]
        x2d, info = hb.to_device_2d(x)
        for fmt in ALL:
            y = hb.unflatten(hb.quantize(x2d, fmt), info).cpu().numpy()
            want = d[f"{name}_y_{fmt}"]
            if info[0] == "vector":  # the reference quantises the flat vector; groups of 16 coincide
                pass
            assert y.shape == want.shape, (name, fmt)
            assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (name, fmt)


def test_quantize_exponent_range_borders():
    """K2/K3's float-domain rounding applies for shared exponents 24..231 and the literal uint32 route outside: groups
    sitting on both sides of both borders, wide in-group spreads, exact ties and saturating values — y bits equal the
    oracle's for every format, through K2 (one format) and K3 (a map mixing all four)."""
    rng = np.random.default_rng(23)
    rows = []
    for e in (1, 2, 7, 22, 23, 24, 25, 26, 60, 127, 200, 229, 230, 231, 232, 233, 253, 254):
        for rep in range(2):
            man = (1.0 + rng.random(16)).astype(np.float32)
            spread = rng.integers(0, 26, size=16)
            spread[rng.integers(0, 16)] = 0                      # one element carries the shared exponent
            sign = np.where(rng.random(16) < 0.5, -1.0, 1.0)
            g = np.ldexp(man * sign, (e - 127) - spread).astype(np.float32)
            if rep:                                               # ties / saturation / zeros inside the group
                g[1] = np.ldexp(np.float32(1.9999999), e - 127)
                g[2] = np.ldexp(np.float32(1.5), e - 127 - 7)
                g[3] = 0.0
                g[4] = np.ldexp(np.float32(-1.0078125), e - 127)
            rows.append(g)
    with np.errstate(all="ignore"):
        x = np.stack(rows).astype(np.float32).reshape(-1, 16)
        x = np.tile(x, (1, 2))                                    # 32 columns: one tile wide, 36 rows
        want = {f: orc.quantize_weight_values(x, f).view(np.uint32) for f in ALL}
    for f in ALL:
        assert np.array_equal(bits(hb.quantize(dev(x), f)), want[f]), f
    amap = rng.integers(0, 4, size=(2, 1)).astype(np.int8)
    amap[0, 0], amap[1, 0] = 1, 3
    y = bits(hb.apply_assignment(dev(x), amap))
    for tr in range(2):
        sl = slice(32 * tr, min(32 * (tr + 1), x.shape[0]))
        assert np.array_equal(y[sl], want[ALL[int(amap[tr, 0])]][sl]), tr


@pytest.mark.parametrize("kind,shape", [
    ("normal_bf16", (256, 256)), ("heavy_bf16", (192, 160)), ("normal_f32", (130, 200)), ("heavy_f32", (50, 70)),
    ("heavy_f32", (33, 17)), ("normal_f32", (1, 1)), ("heavy_bf16", (257, 95)), ("normal_bf16", (64, 4096)),
])
def test_tile_stats_bit_exact(kind, shape):
    x = gen(kind, 42, shape)
    for fm in (ALL, ["bfp8", "bfp2"], ["bf16"], ["bfp4"]):
        mask = hb.fmt_mask(fm)
        want = orc.tile_stats(x, fm)
        got = hb.tile_stats(dev(x), mask).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (kind, shape, fm)
        if kind.endswith("bf16"):  # bf16 STORAGE must give the same records as the fp32 view of the same values
            got16 = hb.tile_stats(dev(x, bf16=True), mask).cpu().numpy()
            assert np.array_equal(got16.view(np.uint64), want.view(np.uint64)), (kind, shape, fm, "bf16 storage")


def test_tile_stats_specials(golden_dir):
    """Inf/NaN/denormal/wrap-around groups: records equal the oracle's, NaN == NaN."""
    x = np.load(golden_dir / "f1_quantize_kat.npz")["x_bits"].view(np.float32)
    with np.errstate(all="ignore"):
        want = orc.tile_stats(x, ALL)
    got = hb.tile_stats(dev(x), 0xF).cpu().numpy()
    both_nan = np.isnan(want) & np.isnan(got)
    assert np.array_equal(np.where(both_nan, 0, got.view(np.uint64)), np.where(both_nan, 0, want.view(np.uint64)))


def test_tile_stats_strided_and_batched():
    x = gen("heavy_bf16", 5, (96, 320))
    big = dev(x, bf16=True)
    view = big[:, 64:256]  # ld = 320, cols = 192, 16-byte aligned start
    want = orc.tile_stats(x[:, 64:256], ALL)
    assert np.array_equal(hb.tile_stats(view, 0xF).cpu().numpy().view(np.uint64), want.view(np.uint64))
    view2 = big[:, 3:100]  # misaligned start → scalar loads
    want2 = orc.tile_stats(x[:, 3:100], ALL)
    assert np.array_equal(hb.tile_stats(view2, 0xF).cpu().numpy().view(np.uint64), want2.view(np.uint64))
    xs = np.stack([gen("normal_bf16", s, (64, 96)) for s in range(5)])
    got = hb.tile_stats_batched(dev(xs, bf16=True), 0xF).cpu().numpy()
    for i in range(5):
        assert np.array_equal(got[i].view(np.uint64), orc.tile_stats(xs[i], ALL).view(np.uint64))


def test_apply_assignment_matches_oracle():
    rng = np.random.default_rng(0)
    for kind, shape in (("heavy_f32", (130, 200)), ("normal_bf16", (96, 64)), ("heavy_f32", (1003,))):
        x = gen(kind, 9, shape)
        x2d, info = hb.to_device_2d(x)
        th, tw = hb.tiles_hw(*x2d.shape)
        a = rng.integers(0, 4, size=(th, tw)).astype(np.int8)
        y = hb.unflatten(hb.apply_assignment(x2d, a), info).cpu().numpy()
        want = orc.apply_assignment(x, a)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (kind, shape)


def test_greedy_maps_from_gpu_stats_match_golden(golden_dir):
    d = np.load(golden_dir / "f4_greedy.npz")
    meta = json.loads((golden_dir / "golden_meta.json").read_text())["f4"]
    for name, m in meta.items():
        x = gen(m["kind"], m["seed"], tuple(m["shape"]))
        x2d, _ = hb.to_device_2d(x)
        fm = [f for f in ALL if f in m["formats"]]
        mask = hb.fmt_mask(fm)
        stats = hb.tile_stats(x2d, mask).cpu().numpy()
        scan = hb.GreedyScan(stats, mask, m["metric"], m["threshold"], float(x.size), m["formats"][0])
        rng = np.random.default_rng(m["algo_seed"])
        for fmt in m["formats"]:
            cand = np.where(scan.fixed() == 0)[0]
            if cand.size == 0:
                break
            scan.run_pass(fmt, rng.permutation(cand))
        want = d[f"{name}_assign"]
        assert np.array_equal(scan.assignment().reshape(want.shape), want), name
        cols = hb.columns_from_stats(stats, mask, scan.assignment(), x.size)
        ref = d[f"{name}_cols"]
        tol = 1e-6 if x.size <= 65536 else 2e-5  # the reference's float32 pcc is noisy above 256x256
        assert abs(cols["pcc"] - ref[0]) <= tol and abs(cols["mae"] - ref[1]) <= 1e-6 and abs(cols["atol"] - ref[2]) <= 1e-6, name


@pytest.mark.parametrize("kind,shape,scale", [
    ("normal_bf16", (32, 128), 1.0), ("heavy_bf16", (96, 256), 1.0), ("heavy_bf16", (64, 384), 2.0 ** 30),
    ("heavy_bf16", (64, 128), 2.0 ** -60), ("normal_bf16", (128, 4096), 1.0), ("heavy_bf16", (32, 128), 2.0 ** 70),
])
def test_fast_bf16_kernel_bit_exact(kind, shape, scale):
    """bf16 storage with whole 32x128 units takes tile_stats_bf16_fast (exact-integer route); its records
    must equal the oracle's literal float32-term / float64-sum records bit for bit, for every mask."""
    x = (gen(kind, 77, shape) * np.float32(scale)).astype(np.float32)
    xb = dev(x, bf16=True)
    for fm in (ALL, ["bfp8", "bfp4", "bfp2"], ["bf16", "bfp4"], ["bfp2"]):
        want = orc.tile_stats(x, fm)
        got = hb.tile_stats(xb, hb.fmt_mask(fm)).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (kind, shape, scale, fm)


def test_fast_bf16_kernel_fallback_groups():
    """Groups the exact-integer route cannot take (zeros, values > 15 binades below the group maximum,
    denormals, Inf/NaN, huge/tiny exponents) must come out identical through the literal fallback."""
    rng = np.random.default_rng(3)
    x = gen("heavy_bf16", 5, (64, 256)).copy()
    x[0, :16] = 0.0                                    # all-zero group
    x[1, 3] = 0.0                                      # one exact zero
    x[2, 16:32] = x[2, 16:32] * np.float32(2.0 ** -20) # tiny group next to a normal one
    x[3, 5] = np.float32(2.0 ** -40)                   # element 16+ binades below the maximum
    x[4, :16] = np.float32(1e-40)                      # bf16 denormals
    x[5, 7] = np.inf
    x[6, 9] = np.nan
    x[7, :16] = np.float32(3.0e38)
    x[8, :16] = np.float32(2.0 ** -100)
    x[9, 16:32] = np.where(rng.random(16) < 0.5, 0.0, x[9, 16:32])
    x[40:, 128:] = 0.0                                 # zero tile block
    xb = torch.from_numpy(x).to(torch.bfloat16)       # host cast; the oracle sees exactly these bf16 values
    x = xb.float().numpy()
    with np.errstate(all="ignore"):
        want = orc.tile_stats(x, ALL)
    got = hb.tile_stats(xb.cuda(), 0xF).cpu().numpy()
    both_nan = np.isnan(want) & np.isnan(got)
    assert np.array_equal(np.where(both_nan, 0, got.view(np.uint64)), np.where(both_nan, 0, want.view(np.uint64)))


def _nan_eq(got, want):
    both_nan = np.isnan(want) & np.isnan(got)
    return np.array_equal(np.where(both_nan, 0, got.view(np.uint64)), np.where(both_nan, 0, want.view(np.uint64)))


def test_direct_kernel_every_mask_and_edge_groups():
    """mtq_direct.hip (float32 storage; ragged / unaligned bf16): every format subset, tail-class elements, zeros,
    shared exponents at and beyond the borders of the exact route's range [80,180], specials — all bit-identical to the
    oracle's literal route, and to the literal GPU kernel where NaN payloads are involved."""
    rng = np.random.default_rng(11)
    x = gen("heavy_f32", 7, (70, 200)).copy()           # ragged in both directions: zero pads inside edge tiles
    x[0, :16] = 0.0                                      # all-zero group inside a live tile
    x[1, 3] = 0.0
    x[1, 4] = -0.0
    x[2, 16:32] *= np.float32(2.0 ** -20)
    x[3, 5] = np.float32(2.0 ** -40)                     # 16+ binades below its group's maximum: tail class
    x[3, 6] = np.float32(-(2.0 ** -30))
    x[4, 32:48] = (rng.standard_normal(16) * 2.0 ** -15).astype(np.float32) * x[4, 32]   # d around the 14/15 class border
    x[5, :16] = np.float32(1e-40)                        # denormals only (E = 0, non-zero): literal redo
    x[6, 7] = np.inf
    x[7, 9] = np.nan
    x[8, :16] = np.float32(3.0e38)
    for r, e in ((9, 79), (10, 80), (11, 180), (12, 181)):  # borders of the exact route
        x[r, 48:64] = (1.0 + rng.random(16)).astype(np.float32) * np.float32(2.0 ** (e - 127)) * np.where(rng.random(16) < 0.5, -1, 1)
    x[13, 64:80] = np.ldexp(np.float32(1.0), -np.arange(16, dtype=np.int32) * 2).astype(np.float32)  # one value per 2 binades
    x[14, 64:80] = np.float32(1.9999999)                 # saturating round-up in every format
    x[40:64, 128:160] = 0.0                              # an all-zero tile
    for fm_bits in range(1, 16):
        fm = [f for i, f in enumerate(ALL) if fm_bits >> i & 1]
        with np.errstate(all="ignore"):
            want = orc.tile_stats(x, fm)
        got = hb.tile_stats(dev(x), fm_bits).cpu().numpy()
        assert _nan_eq(got, want), fm
    # unaligned rows (ld not a multiple of 4 elements) and a column offset: scalar loads, same records
    big = torch.zeros((70, 203), dtype=torch.float32, device="cuda")
    big[:, 3:] = dev(x)
    with np.errstate(all="ignore"):
        assert _nan_eq(hb.tile_stats(big[:, 3:], 0xF).cpu().numpy(), orc.tile_stats(x, ALL))
    # bf16 STORAGE on the same route (ragged shape → not the LDS-staged kernel)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    x16 = xb.float().numpy()
    for fm_bits in (0xF, 0x1, 0x6, 0x9):
        fm = [f for i, f in enumerate(ALL) if fm_bits >> i & 1]
        with np.errstate(all="ignore"):
            want = orc.tile_stats(x16, fm)
        assert _nan_eq(hb.tile_stats(xb.cuda(), fm_bits).cpu().numpy(), want), fm


def test_direct_kernel_mid_size_f32_and_batched():
    """gpt2-like (768x2304) and DeepSeek-like (fp8 values x block scales) float32 tensors, plus a batched launch."""
    x = gen("normal_f32", 21, (768, 2304))
    assert np.array_equal(hb.tile_stats(dev(x), 0xF).cpu().numpy().view(np.uint64), orc.tile_stats(x, ALL).view(np.uint64))
    rng = np.random.default_rng(5)
    m, e = np.frexp(rng.standard_normal((512, 640)))
    base = np.ldexp(np.round(m * 16) / 16, e)
    sc = np.exp(rng.standard_normal((4, 5))) * 0.01
    y = (base * np.repeat(np.repeat(sc, 128, 0), 128, 1)).astype(np.float32)
    assert np.array_equal(hb.tile_stats(dev(y), 0xE).cpu().numpy().view(np.uint64), orc.tile_stats(y, ["bfp8", "bfp4", "bfp2"]).view(np.uint64))
    xs = np.stack([gen("heavy_f32", s, (96, 160)) for s in range(5)])
    got = hb.tile_stats_batched(dev(xs), 0xF).cpu().numpy()
    for i in range(5):
        assert np.array_equal(got[i].view(np.uint64), orc.tile_stats(xs[i], ALL).view(np.uint64)), i


def test_direct_kernel_full_size_properties():
    """A DeepSeek-R1 layer-0 shape at full size (q_b_proj 24576 x 1536, float32 after the fp8 x scale dequantisation;
    BASELINE.json configs[2]): size-independent properties of the float32 route — checksum of checksums, power-of-two
    homogeneity bit for bit, row-block independence, batched == single — plus the oracle on a 1024-row crop."""
    g = torch.Generator().manual_seed(3)
    rows, cols = 24576, 1536
    m, e = torch.frexp(torch.randn((rows, cols), generator=g))
    base = torch.ldexp(torch.round(m * 16) / 16, e)                          # fp8-e4m3-like significands
    scale = torch.exp(torch.randn((rows // 128, cols // 128), generator=g)) * 0.01
    x = (base * scale.repeat_interleave(128, 0).repeat_interleave(128, 1)).float().contiguous()
    xd = x.cuda()
    got = hb.tile_stats(xd, 0xF).cpu().numpy()
    assert got.shape == (rows // 32 * (cols // 32), 22) and not np.isnan(got).any()
    x64 = x.double()
    assert abs(got[:, 0].sum() - float(x64.sum())) <= 1e-9 * float(x64.abs().sum())
    assert abs(got[:, 1].sum() - float((x64 * x64).sum())) <= 1e-7 * float((x64 * x64).sum())   # each x*x is a float32 product
    crop = x[4096:5120].numpy()
    th = cols // 32
    want = orc.tile_stats(crop, ALL)
    assert np.array_equal(got[128 * th:160 * th].view(np.uint64), want.view(np.uint64))   # tile rows 128..159 = rows 4096..5119
    got4 = hb.tile_stats(xd * 4.0, 0xF).cpu().numpy()                        # x·2^k is exact: moments scale by 2^k / 4^k
    sc = np.ones(22)
    sc[[0, 2, 5, 6, 7, 10, 11, 12, 15, 16, 17, 20, 21]] = 4.0
    sc[[1, 3, 4, 8, 9, 13, 14, 18, 19]] = 16.0
    assert np.array_equal(got4, got * sc)
    xs = xd.clone()
    xs[0:32], xs[320:352] = xd[320:352], xd[0:32]                             # swap two tile rows: their records swap
    gs = hb.tile_stats(xs, 0xF).cpu().numpy().reshape(rows // 32, th, 22)
    g0 = got.reshape(rows // 32, th, 22)
    assert np.array_equal(gs[0], g0[10]) and np.array_equal(gs[10], g0[0]) and np.array_equal(gs[11:], g0[11:])
    gb = hb.tile_stats_batched(torch.stack([xd[:2048], xs[:2048]]), 0xE).cpu().numpy()
    assert np.array_equal(gb[0], hb.tile_stats(xd[:2048], 0xE).cpu().numpy())
    assert np.array_equal(gb[1], hb.tile_stats(xs[:2048], 0xE).cpu().numpy())


def test_fast_and_generic_kernels_agree_batched():
    xs = np.stack([gen("normal_bf16", s, (64, 256)) for s in range(6)])
    got = hb.tile_stats_batched(dev(xs, bf16=True), 0xF).cpu().numpy()
    for i in range(6):
        assert np.array_equal(got[i].view(np.uint64), orc.tile_stats(xs[i], ALL).view(np.uint64)), i


def test_full_size_parity_and_properties():
    """BASELINE.json configs[1] size (4096x4096 bf16) and a Llama-3 MLP shape: records bit-identical to the oracle,
    plus size-independent properties of the exact-integer route (power-of-two homogeneity, tile independence,
    batched == single, checksum of checksums)."""
    from quantization_analysis_amd.compression_algorithms import create_algorithm
    from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer

    g = torch.Generator().manual_seed(0)
    xb = (torch.randn((4096, 4096), generator=g) * 0.02).to(torch.bfloat16)
    x = xb.float().numpy()
    xd = xb.cuda()
    got = hb.tile_stats(xd, 0xF).cpu().numpy()
    want = orc.tile_stats(x, ALL)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # checksum of checksums: Σ over tiles of Σx / Σx² equals the float64 sums of the tensor
    assert abs(got[:, 0].sum() - x.astype(np.float64).sum()) <= 1e-9 * np.abs(x).astype(np.float64).sum()
    assert abs(got[:, 1].sum() - (x.astype(np.float64) ** 2).sum()) <= 1e-12 * (x.astype(np.float64) ** 2).sum()
    # power-of-two homogeneity: x·2^k is exact in bf16; first moments scale by 2^k, second moments by 4^k, bit for bit
    got8 = hb.tile_stats((xd.float() * 8.0).to(torch.bfloat16), 0xF).cpu().numpy()
    scale = np.ones(22)
    scale[[0, 2, 5, 6, 7, 10, 11, 12, 15, 16, 17, 20, 21]] = 8.0
    scale[[1, 3, 4, 8, 9, 13, 14, 18, 19]] = 64.0
    assert np.array_equal(got8, got * scale)
    # tile independence: swapping two tile rows swaps their records
    xs = xd.clone()
    xs[0:32], xs[64:96] = xd[64:96], xd[0:32]
    gs = hb.tile_stats(xs, 0xF).cpu().numpy().reshape(128, 128, 22)
    g0 = got.reshape(128, 128, 22)
    assert np.array_equal(gs[0], g0[2]) and np.array_equal(gs[2], g0[0]) and np.array_equal(gs[3:], g0[3:])
    # batched launch == single launches
    gb = hb.tile_stats_batched(torch.stack([xd, xs]), 0xF).cpu().numpy()
    assert np.array_equal(gb[0], got) and np.array_equal(gb[1].reshape(128, 128, 22), gs)
    # full greedy search: map identical to the oracle's at full size
    res = create_algorithm("mixed-tile-greedy", {"metric": "pcc", "threshold": 0.999, "seed": 123, "materialize_y": False}).run(
        xd, ALL, Quantizer("hip"), None)[0]
    want_a, want_counts, _st = orc.greedy(x, ALL, "pcc", 0.999, 123)
    assert np.array_equal(res.meta["assignment"], want_a) and res.tile_counts == want_counts
    # a Llama-3-8B MLP shape (14336 x 4096), heavier tails
    xl = (torch.randn((14336, 4096), generator=g) * 0.02 * torch.exp(0.5 * torch.randn((14336, 4096), generator=g))).to(torch.bfloat16)
    gl = hb.tile_stats(xl.cuda(), 0xE).cpu().numpy()
    assert np.array_equal(gl.view(np.uint64), orc.tile_stats(xl.float().numpy(), ["bfp8", "bfp4", "bfp2"]).view(np.uint64))


def test_sparse_tensors_and_concurrent_streams():
    """(1) Pruned weights: half of the shared-exponent groups, some whole tiles and one whole tensor are zero — zero groups
    must not send tiles to the literal fix-up, and the records stay bit-identical.  (2) K1 launches racing on four streams
    (each launch claims its units from its own slot of the device counter ring) give the same records as serial launches."""
    rng = np.random.default_rng(17)
    x = gen("normal_bf16", 9, (128, 512)).copy()
    keep = rng.random((128, 32)) < 0.5
    x *= np.repeat(keep, 16, axis=1)
    x[32:64, 128:192] = 0.0
    want = orc.tile_stats(x, ALL)
    got = hb.tile_stats(dev(x, bf16=True), 0xF).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    zeros = torch.zeros((64, 256), dtype=torch.bfloat16, device="cuda")
    assert not hb.tile_stats(zeros, 0xF).cpu().numpy().any()
    assert not hb.tile_stats(zeros.float(), 0xF).cpu().numpy().any()

    xs = [dev(gen("heavy_bf16", 40 + i, (256, 512)), bf16=True) for i in range(4)]
    xf = [dev(gen("heavy_f32", 50 + i, (160, 224))) for i in range(4)]
    serial = [hb.tile_stats(t, 0xF).cpu().numpy() for t in xs + xf]
    streams = [torch.cuda.Stream() for _ in range(4)]
    outs = [None] * 8
    torch.cuda.synchronize()
    for rep in range(6):
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs[k] = hb.tile_stats(xs[k], 0xF)
                outs[4 + k] = hb.tile_stats(xf[k], 0xF)
        torch.cuda.synchronize()
        for k in range(8):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint64), serial[k].view(np.uint64)), (rep, k)


def test_device_decisions_equal_host_decisions(golden_dir):
    """K4 / per-tile scores / column sums evaluated on the device from device-resident records: the same double
    arithmetic as the host functions (csrc/mtq_decide.hpp) — scores and maps bit for bit, knife-edge sets equal, the
    tree-ordered column sums within 1e-13 relative of the tile-ordered host sums."""
    meta = json.loads((golden_dir / "golden_meta.json").read_text())["f5"]
    d = np.load(golden_dir / "f5_threshold.npz")
    for name, m in meta.items():
        x = d[f"{name}_x"]
        x2d, _info = hb.to_device_2d(x)
        fm = [f for f in ALL if f in m["formats"]]
        mask = hb.fmt_mask(fm)
        sdev = hb.tile_stats(x2d, mask)
        shost = sdev.cpu().numpy()
        for metric in ("pcc", "mae", "atol"):
            got = hb.tile_scores_device(sdev, mask, metric).cpu().numpy()
            want = hb.tile_scores(shost, mask, metric)
            both_nan = np.isnan(got) & np.isnan(want)
            assert np.array_equal(np.where(both_nan, 0, got.view(np.uint64)), np.where(both_nan, 0, want.view(np.uint64))), (name, metric)
        a_dev, k_dev = hb.threshold_assign_device(sdev, mask, m["formats"], m["metric"], m["threshold"], 2e-6)
        a_host, k_host = hb.threshold_assign(shost, mask, m["formats"], m["metric"], m["threshold"], 2e-6)
        assert np.array_equal(a_dev, a_host) and np.array_equal(k_dev, k_host), name
        amap = d[f"{name}_assign"].reshape(-1)
        c_dev = hb.columns_from_stats_device(sdev, mask, amap, float(x.size))
        c_host = hb.columns_from_stats(shost, mask, amap, float(x.size))
        assert c_dev["atol"] == c_host["atol"]
        for key in ("pcc", "mae"):
            assert abs(c_dev[key] - c_host[key]) <= 1e-13 * max(1.0, abs(c_host[key])), (name, key)
    # a big one: 4096x4096 bf16, identity records (BFP slots only)
    g = torch.Generator().manual_seed(5)
    xb = (torch.randn((4096, 4096), generator=g) * 0.02).to(torch.bfloat16).cuda()
    sdev = hb.tile_stats(xb, 0xE)
    ident = 0xE | hb.MASK_BF16_IDENTITY
    got = hb.tile_scores_device(sdev, ident, "pcc").cpu().numpy()
    want = hb.tile_scores(sdev.cpu().numpy(), ident, "pcc")
    assert got.shape == (4, 16384) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    thr = float(np.median(got[2]))                         # the median bfp4 tile score: a mixed map with knife-edge tiles
    a_dev, k_dev = hb.threshold_assign_device(sdev, ident, ALL, "pcc", thr, 2e-6)
    a_host, k_host = hb.threshold_assign(sdev.cpu().numpy(), ident, ALL, "pcc", thr, 2e-6)
    assert np.array_equal(a_dev, a_host) and np.array_equal(k_dev, k_host) and len(set(a_dev.tolist())) >= 2 and k_dev.size > 0
    with pytest.raises(hb.MtqError):
        hb.columns_from_stats_device(hb.tile_stats(xb[:64, :128], 0x2), 0x2, np.full(8, 3, dtype=np.int8), 8192.0)


def test_knife_tiles_device_lists_fetches_and_quantises():
    """mtq_knife_tiles_device against the steps it replaces (an indexed gather of the flagged tiles and K2 per format on them): the listed
    ids are exactly the flagged tiles, every listed tile's values and reconstructions are the same bits; ragged shapes (zero pads), bf16
    and float32 storage, a list shorter than the number of flagged tiles (the count still says how many there were)."""
    import torch

    from quantization_analysis_amd.pipeline import ThresholdPipeline

    rng = np.random.default_rng(5)
    for kind, shape, bf16 in (("normal_bf16", (128, 256), True), ("heavy_f32", (100, 72), False), ("heavy_bf16", (96, 160), True)):
        xs = dev(np.stack([gen(kind, 80 + i, shape) for i in range(3)]), bf16=bf16)
        th, tw = hb.tiles_hw(*shape)
        tiles = th * tw
        near = (rng.random(3 * tiles) < 0.2).astype(np.int8) * rng.integers(1, 15, 3 * tiles).astype(np.int8)
        flagged = np.flatnonzero(near)
        near_dev = torch.from_numpy(near).cuda()
        pipe = ThresholdPipeline(ALL, "pcc", 0.99)
        for cap in (flagged.size + 5, max(flagged.size - 3, 1), 0):
            lst = torch.full((cap + 1,), -7, dtype=torch.int64, device="cuda")
            out = torch.full((1 + len(ALL), cap, 32, 32), float("nan"), dtype=torch.float32, device="cuda")
            hb.knife_tiles_device(xs, near_dev, ALL, cap, lst, out)
            got = lst.cpu().numpy()
            assert got[cap] == flagged.size
            k = min(cap, flagged.size)
            ids = got[:k]
            assert len(set(ids.tolist())) == k and set(ids.tolist()) <= set(flagged.tolist())
            if cap >= flagged.size:
                assert np.array_equal(np.sort(ids), flagged)
            if k:
                want = pipe._knife_tiles_device(xs, torch.from_numpy(ids).cuda(), tiles, tw).cpu().numpy()
                assert np.array_equal(out[:, :k].cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, cap)
        pipe.close()


def test_threshold_pipeline_matches_oracle():
    """ThresholdPipeline (records never leave the GPU): maps and counts equal the oracle's threshold search tensor by tensor,
    columns within 1e-6 of the float32 reference columns; a threshold placed on a tile score exercises the knife-edge path."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    for kind, shape, bf16, cap in (("normal_bf16", (128, 256), True, None), ("heavy_f32", (96, 160), False, None), ("normal_bf16", (100, 72), True, None),
                                   ("heavy_f32", (96, 160), False, 0), ("normal_bf16", (128, 256), True, 1)):
        xs = np.stack([gen(kind, 60 + i, shape) for i in range(5)])
        s4 = orc.threshold_scores(xs[0], ALL, "pcc")["bfp4"]
        for thr in (0.99, float(np.sort(s4)[len(s4) // 2])):          # the second one IS a tile's float32 score
            pipe = ThresholdPipeline(ALL, "pcc", thr, chunk=2)
            if cap is not None:
                pipe.knife_cap = cap          # a knife-edge list too short for the batch: the extra round trip, same maps
            res = pipe.run(dev(xs, bf16=bf16))
            assert [r.index for r in res] == list(range(5))
            pipe.chunk = 8                    # the whole batch as one chunk: main stream only, the listed tiles fetched after the list
            for r1, r2 in zip(res, pipe.run(dev(xs, bf16=bf16))):
                assert np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts and (r1.pcc, r1.mae, r1.atol) == (r2.pcc, r2.mae, r2.atol)
            for i, r in enumerate(res):
                a, counts, _sc = orc.threshold(xs[i], ALL, "pcc", thr)
                assert np.array_equal(r.assignment, a) and r.counts == counts, (kind, thr, i)
                y = orc.apply_assignment(xs[i], a)
                # float64 moments against a float64 two-pass Pearson (1e-7: the float32 products inside the sums), and
                # against the reference's own float32 value (its BLAS noise is ~1e-6 on a 32K-element tensor)
                assert abs(r.pcc - orc.pearson_corr_f64(xs[i], y)) <= 1e-7 and abs(r.pcc - orc.pearson_corr(xs[i], y)) <= 3e-6
                assert abs(r.mae - float(np.mean(np.abs(xs[i] - y)))) <= 1e-6
                assert r.atol == float(np.max(np.abs(xs[i] - y)))
        assert pipe.knife_tiles >= 1


@pytest.mark.gpu
def test_threshold_run_batches_equals_run():
    """ThresholdPipeline.run_batches over batches of different shapes and storage types, a vector as a (n/32, 32) matrix with its element
    count among them, with a threshold ON a tile's float32 score (knife-edge tiles in flight while later batches are enqueued): per batch the
    results of run(), and the oracle's maps."""
    import torch

    from quantization_analysis_amd.pipeline import ThresholdPipeline

    v = gen("normal_bf16", 77, (1000,))
    vm = np.zeros((32 * 32,), dtype=np.float32)
    vm[:1000] = v
    mats = [np.stack([gen("normal_bf16", 70 + i, (128, 256)) for i in range(3)]), np.stack([gen("heavy_f32", 80 + i, (96, 160)) for i in range(2)]),
            np.stack([gen("normal_bf16", 90, (100, 72))])]
    s4 = orc.threshold_scores(mats[0][0], ALL, "pcc")["bfp4"]
    for thr in (0.99, float(np.sort(s4)[len(s4) // 2])):
        batches = [(dev(mats[0], bf16=True), None), (dev(mats[1], bf16=False), None), (dev(mats[2], bf16=True), None),
                   (torch.from_numpy(vm).cuda().to(torch.bfloat16).view(1, 32, 32), 1000)]
        with ThresholdPipeline(ALL, "pcc", thr, chunk=2) as pipe:
            got = pipe.run_batches(batches)
            want = [pipe.run(x, n) for x, n in batches]
        for g, w in zip(got, want):
            assert len(g) == len(w)
            for r1, r2 in zip(g, w):
                assert np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts and (r1.pcc, r1.mae, r1.atol) == (r2.pcc, r2.mae, r2.atol)
        for b, m in enumerate(mats):
            for i in range(m.shape[0]):
                a, counts, _sc = orc.threshold(m[i], ALL, "pcc", thr)
                assert np.array_equal(got[b][i].assignment, a) and got[b][i].counts == counts, (thr, b, i)
        a, counts, _sc = orc.threshold(v, ALL, "pcc", thr)
        assert np.array_equal(got[3][0].assignment, a) and got[3][0].counts == counts


def test_threshold_pipeline_refuses_inner_strided_batches():
    """A batch whose rows are not contiguous (x[:, :, ::2]) is refused by the one-call enqueue, on its own and through run_batches,
    instead of being read as if its rows were."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline

    x = dev(np.stack([gen("normal_bf16", 60 + i, (64, 256)) for i in range(2)]), bf16=True)[:, :, ::2]
    with ThresholdPipeline(ALL, "pcc", 0.999) as pipe:
        with pytest.raises(hb.MtqError, match="contiguous rows"):
            pipe.enqueue(x)
        with pytest.raises(hb.MtqError, match="contiguous rows"):
            pipe.run_batches([x])


def _ragged_inputs(bf16: bool):
    """Matrices of assorted shapes (whole tiles, ragged edges, one tile, a (n/32, 32) vector form, a strided view), some with values the
    exact routes hand to the literal fix-up (NaN, inf, huge, subnormal)."""
    kind = "heavy_bf16" if bf16 else "heavy_f32"
    hosts = [gen(kind, 300 + i, sh) for i, sh in enumerate([(70, 100), (32, 32), (48, 32), (256, 512), (33, 17), (64, 1000)])]
    hosts[0][3, 5], hosts[0][40, 99] = np.nan, np.inf
    hosts[3][100, 200:216] = np.float32(3e38)
    hosts[3][7, 64:80] = np.float32(1e-41)
    hosts[5][:, 500:] = 0.0
    wide = dev(np.concatenate([hosts[5], hosts[5]], axis=1), bf16)
    mats = [dev(h, bf16) for h in hosts[:5]] + [wide[:, :1000]]                     # the last: rows 2000 elements apart
    return hosts, mats


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mask", [0xF, 0xE, 0x6])
def test_tile_stats_ragged_equals_per_matrix(bf16, mask):
    """mtq_tile_stats_ragged: one launch over matrices of any shapes — the records of mtq_tile_stats matrix by matrix, bit for bit
    (marked tiles included: the fix-up reads the same table).  The literal kernel's form: test_pipeline_under_force_generic_switch."""
    hosts, mats = _ragged_inputs(bf16)
    got = hb.tile_stats_ragged(mats, mask).cpu().numpy().view(np.int64)
    at = 0
    for h, m in zip(hosts, mats):
        want = hb.tile_stats(m, mask).cpu().numpy().view(np.int64)
        assert np.array_equal(got[at:at + want.shape[0]], want), (h.shape, bf16, mask)
        at += want.shape[0]
    assert at == got.shape[0]
    with pytest.raises(hb.MtqError):
        hb.tile_stats_ragged(mats * 5, mask)                                          # 30 matrices: more than a table holds
    with pytest.raises(hb.MtqError):
        hb.tile_stats_ragged([mats[0], mats[1].float() if bf16 else mats[1].to(torch.bfloat16)], mask)   # two storage types


def test_column_sums_ragged_equals_per_tensor():
    """mtq_column_sums_device_ragged: every tensor of a ragged batch summed in the order mtq_column_sums_device uses for it alone."""
    import ctypes

    _hosts, mats = _ragged_inputs(False)
    mats = [m for m in mats] + [dev(gen("normal_f32", 5, (2048, 2048)))]               # 4096 tiles: 16 partial blocks
    per = [hb.tiles_hw(*m.shape)[0] * hb.tiles_hw(*m.shape)[1] for m in mats]
    recs = hb.tile_stats_ragged(mats, 0xF)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    maps = torch.randint(0, 4, (sum(per),), generator=g, device="cuda").to(torch.int8)
    sn = int(hb.lib().mtq_columns_scratch_doubles())
    scratch = torch.zeros((len(mats), sn), dtype=torch.float64, device="cuda")
    hb.check(hb.lib().mtq_column_sums_device_ragged(recs.data_ptr(), (ctypes.c_int64 * len(per))(*per), len(per), 0xF, maps.data_ptr(), scratch.data_ptr(), None))
    at = 0
    for j, t in enumerate(per):
        one = torch.zeros((sn,), dtype=torch.float64, device="cuda")
        hb.check(hb.lib().mtq_column_sums_device(recs[at:at + t].contiguous().data_ptr(), t, 0xF, maps[at:at + t].contiguous().data_ptr(), one.data_ptr(), None))
        a, b = scratch[j, :11].cpu().numpy().view(np.int64), one[:11].cpu().numpy().view(np.int64)
        assert np.array_equal(a, b), (j, t)
        assert np.array_equal(scratch[j, 7:11].cpu().numpy(), np.bincount(maps[at:at + t].cpu().numpy().view(np.uint8), minlength=4).astype(np.float64))
        at += t


@pytest.mark.parametrize("knife_cap", [128, 1])
def test_threshold_ragged_groups(monkeypatch, knife_cap):
    """run_batches with ragged groups (many shapes, two storage types, more matrices than one table holds, `none` rows on request) against
    the same batches with the switch off (a launch chain per batch) and the oracle; knife_cap 1: more knife-edge tiles than the list holds
    (the matrix-by-matrix second trip)."""
    from quantization_analysis_amd.pipeline import ThresholdPipeline
    from quantization_analysis_amd.settings import settings

    shapes = [(70, 100), (32, 32), (96, 160), (33, 17), (64, 200)]
    hosts = [gen("heavy_f32", 400 + i, shapes[i % len(shapes)]) for i in range(27)] + [gen("normal_bf16", 500 + i, shapes[i % len(shapes)]) for i in range(3)]
    s4 = orc.threshold_scores(hosts[2], ALL, "pcc")["bfp4"]
    thr = float(np.sort(s4)[len(s4) // 2])                                              # ON a tile's score: knife-edge tiles exist
    batches = [dev(h, bf16=i >= 27)[None] for i, h in enumerate(hosts)]
    runs = {}
    for ragged in ("1", "0"):
        monkeypatch.setenv("MTQ_THRESHOLD_RAGGED", ragged)
        monkeypatch.setenv("MTQ_KNIFE_CAP", str(knife_cap))
        settings(refresh=True)
        with ThresholdPipeline(ALL, "pcc", thr, chunk=1, pure_formats=("bfp8", "bfp4")) as pipe:
            runs[ragged] = pipe.run_batches(batches)
            assert pipe.knife_tiles > 0
    for i, (a, b) in enumerate(zip(runs["1"], runs["0"])):
        r1, r2 = a[0], b[0]
        assert np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts and (r1.pcc, r1.mae, r1.atol) == (r2.pcc, r2.mae, r2.atol), i
        assert r1.pure == r2.pure and r1.index == 0
        want, counts, _sc = orc.threshold(hosts[i], ALL, "pcc", thr)
        assert np.array_equal(r1.assignment, want) and r1.counts == counts, i


@pytest.mark.parametrize("scan", ["device", "host"])
def test_streamed_pipeline_matches_oracle(scan):
    """GreedyPipeline (what bench.py times), with the scan on the device (csrc/mtq_scan.hip: maps come back, records stay) and
    with records over PCIe + threaded host scans: chunked K1 launches.  bf16 storage takes
    the 17-double records + identity bf16 (MTQ_MASK_BF16_IDENTITY), float32 storage the full records; maps, counts and
    columns equal the oracle's greedy search tensor by tensor, with per-tensor seeds."""
    from quantization_analysis_amd.pipeline import GreedyPipeline

    for kind, shape, bf16 in (("normal_bf16", (128, 256), True), ("heavy_bf16", (96, 160), True), ("heavy_f32", (96, 160), False)):
        xs = np.stack([gen(kind, 30 + i, shape) for i in range(5)])
        seeds = [11, 12, 13, 14, 15]
        pipe = GreedyPipeline(ALL, "pcc", 0.998, 123, chunk=2, workers=3, scan=scan)
        assert pipe.device_scan == (scan == "device")
        try:
            res = pipe.run(dev(xs, bf16=bf16), seeds=seeds)
            res2 = pipe.run(dev(xs, bf16=bf16), seeds=seeds)   # buffers are reused: same answer again
        finally:
            pipe.close()
        assert [r.index for r in res] == list(range(5))
        for i, r in enumerate(res):
            a, counts, st = orc.greedy(xs[i], ALL, "pcc", 0.998, seeds[i])
            assert np.array_equal(r.assignment, a) and r.counts == counts, (kind, i)
            pcc, mae, atol = orc.columns_from_stats(st["stats"], orc.mask_slots(0xF), a, xs[i].size)
            # the pcc pipeline takes its columns from the device (tree-ordered sums): equal to the tile-ordered ones to ~1e-15
            assert abs(r.pcc - pcc) <= 1e-13 and abs(r.mae - mae) <= 1e-13 * max(mae, 1e-30) + 1e-18 and r.atol == atol, (kind, i)
            assert np.array_equal(res2[i].assignment, a)
    # a zero-variance tensor (constant) inside a chunk: the slim scan gives up, the chunk is repeated with the full records
    xs = np.stack([gen("normal_bf16", 90, (64, 128)), np.full((64, 128), 0.5, dtype=np.float32), gen("normal_bf16", 91, (64, 128))])
    pipe = GreedyPipeline(ALL, "pcc", 0.998, 123, chunk=3, workers=2, scan=scan)
    try:
        res = pipe.run(dev(xs, bf16=True))
    finally:
        pipe.close()
    assert pipe.host_fallbacks == (1 if scan == "device" else 0)   # the device scan hands a zero-denominator tensor back to the host scan
    for i, r in enumerate(res):
        a, counts, _st = orc.greedy(xs[i], ALL, "pcc", 0.998, 123)
        assert np.array_equal(r.assignment, a) and r.counts == counts, i
    # the mae metric (Σ|d| decides): on the device too, or over PCIe with the full records
    pipe = GreedyPipeline(ALL, "mae", 3e-4, 123, chunk=2, workers=2, scan=scan)
    assert pipe.device_scan == (scan == "device")
    try:
        res = pipe.run(dev(xs[[0, 2]], bf16=True))
    finally:
        pipe.close()
    for i, r in zip((0, 2), res):
        a, counts, _st = orc.greedy(xs[i], ALL, "mae", 3e-4, 123)
        assert np.array_equal(r.assignment, a) and r.counts == counts, i
    # the atol metric through the pipeline (device: the closed-form walk; host: the sequential scan with its multiplicity bookkeeping)
    pipe = GreedyPipeline(ALL, "atol", 4e-3, 123, chunk=2, workers=2, scan=scan)
    try:
        res = pipe.run(dev(xs[[0, 2]], bf16=True))
    finally:
        pipe.close()
    for i, r in zip((0, 2), res):
        a, counts, _st = orc.greedy(xs[i], ALL, "atol", 4e-3, 123)
        assert np.array_equal(r.assignment, a) and r.counts == counts, i
    # overlapped batches (three record slots): the last batch's results, each batch its own tensors
    b1 = dev(np.stack([gen("normal_bf16", 70 + i, (128, 256)) for i in range(4)]), bf16=True)
    b2x = np.stack([gen("heavy_bf16", 80 + i, (128, 256)) for i in range(4)])
    pipe = GreedyPipeline(ALL, "pcc", 0.998, 123, chunk=3, workers=2, scan=scan)
    try:
        last = pipe.run_steps([b1, dev(b2x, bf16=True), b1, dev(b2x, bf16=True)])
        with pytest.raises(RuntimeError):
            open_ = [pipe.enqueue(b1) for _ in range(pipe.SLOTS)]
            pipe.enqueue(b1)
        for e in open_:
            pipe.finish(e)
    finally:
        pipe.close()
    for i, r in enumerate(last):
        a, counts, _st = orc.greedy(b2x[i], ALL, "pcc", 0.998, 123)
        assert np.array_equal(r.assignment, a) and r.counts == counts, i


def test_streamed_pipeline_mixed_routes_in_one_run():
    """run_batches over batches of three shapes with a tile limit on the device scan: the batch above the limit takes the host route
    (records over PCIe, threaded scans, columns from the flat column buffers), the others the device route, all in flight together
    and prepared up front; pure-format columns (wq's `none` rows) come with both.  Maps, counts and columns equal the oracle's."""
    from quantization_analysis_amd.pipeline import GreedyPipeline

    shapes = [(160, 256), (64, 128), (96, 384)]   # 40, 8 and 36 tiles
    xs = [np.stack([gen("normal_bf16" if k != 1 else "heavy_bf16", 300 + 10 * k + i, shp) for i in range(3 + k)]) for k, shp in enumerate(shapes)]
    pipe = GreedyPipeline(ALL, "pcc", 0.998, 77, chunk=2, workers=3, pure_formats=["bfp8", "bfp2"])
    assert pipe.device_scan
    pipe.device_scan_max_tiles = 36
    pipe.host_chunk_tiles = 80
    pipe.SLOTS = 3
    batches = [dev(x, bf16=True) for x in xs]
    try:
        pipe.prepare(batches)
        routes = [pipe._use_device_scan(-(-s[0] // 32) * -(-s[1] // 32)) for s in shapes]
        assert routes == [False, True, True]
        out = pipe.run_batches(batches)
        again = pipe.run_batches(batches[::-1])[::-1]   # other slots, other column-buffer views: same answers
    finally:
        pipe.close()
    for k, (x3, res) in enumerate(zip(xs, out)):
        assert [r.index for r in res] == list(range(len(x3)))
        for i, r in enumerate(res):
            a, counts, st = orc.greedy(x3[i], ALL, "pcc", 0.998, 77)
            assert np.array_equal(r.assignment, a) and r.counts == counts, (k, i)
            assert np.array_equal(again[k][i].assignment, a), (k, i)
            pcc, mae, atol = orc.columns_from_stats(st["stats"], orc.mask_slots(0xF), a, x3[i].size)
            assert abs(r.pcc - pcc) <= 1e-13 and abs(r.mae - mae) <= 1e-13 * max(mae, 1e-30) + 1e-18 and r.atol == atol, (k, i)
            for f in ("bfp8", "bfp2"):
                code = ALL.index(f)
                p2, m2, a2 = orc.columns_from_stats(st["stats"], orc.mask_slots(0xF), np.full_like(a, code), x3[i].size)
                got = r.pure[f]
                assert abs(got[0] - p2) <= 1e-13 and abs(got[1] - m2) <= 1e-13 * max(m2, 1e-30) + 1e-18 and got[2] == a2, (k, i, f)
                assert again[k][i].pure[f] == got


def test_device_copy_into_pinned_memory():
    """mtq_device_copy_2d (hb.device_copy): how the streamed driver brings maps, counts and sums home — a kernel storing into pinned
    host memory.  Contiguous (16-byte, 8-byte and byte paths), strided rows (the [:, :7] of the column-sum scratch), odd offsets."""
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    for numel, off in ((1 << 20, 0), (4099, 0), (4099, 3), (17, 1)):
        src = torch.randint(-128, 127, (numel + 8,), generator=g, device="cuda", dtype=torch.int8)[off:off + numel]
        dst = torch.zeros((numel + 8,), dtype=torch.int8, pin_memory=True)
        hb.device_copy(dst[off:off + numel], src)
        torch.cuda.synchronize()
        assert torch.equal(dst[off:off + numel], src.cpu()) and int(dst[:off].abs().sum()) == 0 and int(dst[off + numel:].abs().sum()) == 0
    scratch = torch.randn((3, 9, 455), generator=g, device="cuda", dtype=torch.float64)
    host = torch.zeros((3, 9, 7), dtype=torch.float64, pin_memory=True)
    for q in range(3):
        hb.device_copy(host[q, 2:7], scratch[q, 2:7, :7])
    torch.cuda.synchronize()
    assert torch.equal(host[:, 2:7], scratch[:, 2:7, :7].cpu()) and float(host[:, :2].abs().sum()) == 0.0 and float(host[:, 7:].abs().sum()) == 0.0
    dev_dst = torch.zeros((5, 33), dtype=torch.int32, device="cuda")
    src2 = torch.arange(5 * 40, dtype=torch.int32, device="cuda").view(5, 40)
    hb.device_copy(dev_dst, src2[:, 3:36])       # device to device, 4-byte rows at an odd pitch: the byte path
    assert torch.equal(dev_dst, src2[:, 3:36])
    with pytest.raises(ValueError):
        hb.device_copy(dev_dst, src2[:, 3:36].to(torch.int64))
    with pytest.raises(ValueError):
        hb.device_copy(dev_dst.t(), src2[:, 3:36].t())


def test_fast_kernel_strided_view_and_batch_stride():
    """The exact-integer kernel on a column window of a wider matrix (ld > cols) and on a batch whose tensors are
    padded apart (stride > rows*cols): same records as the oracle on the dense copies."""
    x = gen("heavy_bf16", 21, (96, 640))
    big = dev(x, bf16=True)
    view = big[:, 128:512]                      # cols 384 = 3 units, ld 640, 16-byte aligned start
    assert view.stride(0) == 640
    want = orc.tile_stats(np.ascontiguousarray(x[:, 128:512]), ALL)
    assert np.array_equal(hb.tile_stats(view, 0xF).cpu().numpy().view(np.uint64), want.view(np.uint64))
    xs = np.stack([gen("normal_bf16", s, (64, 128)) for s in range(3)])
    buf = torch.zeros((3, 80, 128), dtype=torch.bfloat16, device="cuda")      # 16 spare rows between tensors
    buf[:, :64] = dev(xs, bf16=True)
    out = torch.empty((3, 2 * 4, 22), dtype=torch.float64, device="cuda")
    hb.check(hb.lib().mtq_tile_stats_batched(buf.data_ptr(), hb.DTYPE_BF16, 3, 80 * 128, 64, 128, 128, 0xF, out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i].view(np.uint64), orc.tile_stats(xs[i], ALL).view(np.uint64)), i


# ------------------------------------------------------------------------------------------------------------------
# H1 on the device (csrc/mtq_scan.hip): the whole greedy search where K1 wrote the records
# ------------------------------------------------------------------------------------------------------------------
def _device_scan_vs_host(xs, formats, thr, seeds, mask=None, metric="pcc", numel=None):
    """xs: (count, rows, cols) device tensor.  Device scan maps == host scan maps (same records), status 0.  numel: the tensors'
    element count when the matrices are zero-filled images of shorter vectors (tile_utils.py:96-102; the metric divides by it)."""
    import torch

    ident = xs.dtype == torch.bfloat16 and "bf16" in formats and any(f != "bf16" for f in formats)
    k1 = hb.fmt_mask(formats) & 0xE if ident else hb.fmt_mask(formats)
    dec = k1 | hb.MASK_BF16_IDENTITY if ident else k1
    recs = hb.tile_stats_batched(xs, k1)
    numel = xs.shape[1] * xs.shape[2] if numel is None else int(numel)
    sd = torch.tensor(seeds, dtype=torch.int64, device=xs.device)
    cnt = torch.zeros((xs.shape[0], 4), dtype=torch.int32, device=xs.device)
    maps, status = hb.greedy_scan_device(recs, dec, formats, metric, thr, float(numel), sd, counts_out=cnt)
    torch.cuda.synchronize()
    want, counts, _outs = hb.greedy_run_batch(recs.cpu().numpy(), dec, formats, metric, thr, float(numel), seeds, 4)
    assert status.cpu().tolist() == [0] * xs.shape[0]
    assert np.array_equal(cnt.cpu().numpy(), counts)
    got = maps.cpu().numpy()
    for i in range(xs.shape[0]):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()), formats, thr, seeds[i])
    return got


@pytest.mark.gpu
def test_device_scan_golden_greedy_cases(golden_dir):
    """Every case of golden F4 (the reference's maps: pcc, mae, atol) through K1 + the device scan."""
    import json

    import torch

    meta = json.loads((golden_dir / "golden_meta.json").read_text())["f4"]
    d = np.load(golden_dir / "f4_greedy.npz")
    n = 0
    for name, m in meta.items():
        x = gen(m["kind"], m["seed"], tuple(m["shape"]))
        x2d, info = hb.to_device_2d(torch.from_numpy(x).to(torch.bfloat16) if m["kind"].endswith("bf16") else x)
        # vectors with a ragged last row ((1000,), (1003,), (33,)): the element count is the vector's, not rows*cols (mixed_tile_greedy.py:134)
        got = _device_scan_vs_host(x2d[None].contiguous(), m["formats"], m["threshold"], [m["algo_seed"]], metric=m["metric"], numel=x.size)
        th, tw = hb.tiles_hw(*x2d.shape)
        assert np.array_equal(got[0].reshape(th, tw), d[f"{name}_assign"]), name
        n += 1
    assert n == len(meta) >= 13
    # mae on batches: thresholds around the formats' typical per-tile errors, bf16 storage (identity records) and float32, other orders
    for kind, bf16 in (("normal_bf16", True), ("heavy_f32", False)):
        xs = np.stack([gen(kind, 500 + i, (192, 256)) for i in range(6)])
        xd = dev(xs, bf16=bf16)
        for thr in (5e-5, 2e-4, 1e-3, 1e-2):
            _device_scan_vs_host(xd, ALL, thr, [31 + i for i in range(6)], metric="mae")
        _device_scan_vs_host(xd, ["bfp8", "bfp2"], 3e-4, [5] * 6, metric="mae")
        _device_scan_vs_host(xd, ["bfp4", "bfp8", "bf16"], 3e-4, [9] * 6, metric="mae")
        # atol: order-independent on the device (greedy_atol), sequential with a generator on the host — the same maps, seed after seed
        for thr in (1e-4, 1e-3, 4e-3, 2e-2, 0.2, 10.0):
            _device_scan_vs_host(xd, ALL, thr, [71 + 13 * i for i in range(6)], metric="atol")
        _device_scan_vs_host(xd, ["bfp8", "bfp2"], 2e-2, [5] * 6, metric="atol")
        _device_scan_vs_host(xd, ["bfp4", "bfp8", "bf16"], 2e-2, [9] * 6, metric="atol")


@pytest.mark.gpu
def test_device_search_mae_atol_against_reference_f14(golden_dir):
    """F14: the reference's mixed-tile-greedy maps under mae and atol (1024x768 bf16, 512x640 float32; two seeds each) from K1 + the
    device-side search — the mae instantiation of the scan and the order-free atol walk — by SHA-256, with the counts."""
    import hashlib
    import json

    import torch

    f14 = json.loads((golden_dir / "golden_meta_r2b.json").read_text())["f14"]
    for key, w in f14.items():
        x = gen(w["kind"], w["seed"], tuple(w["shape"]))
        bf16 = w["kind"].endswith("bf16")
        xd = dev(x, bf16=bf16)[None]
        k1 = 0xE if bf16 else 0xF
        dec = k1 | hb.MASK_BF16_IDENTITY if bf16 else k1
        recs = hb.tile_stats_batched(xd, k1)
        sd = torch.tensor([w["algo_seed"]], dtype=torch.int64, device="cuda")
        cnt = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        maps, status = hb.greedy_scan_device(recs, dec, ALL, w["metric"], w["threshold"], float(x.size), sd, counts_out=cnt)
        assert int(status.cpu()[0]) == 0, key
        a = maps.cpu().numpy()[0].reshape(w["assign_shape"])
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == w["assign_sha256"], key
        assert cnt.cpu().numpy()[0].tolist() == w["counts"], key


@pytest.mark.gpu
def test_device_scan_headline_tensor_and_batches(golden_dir):
    """The 4096x4096 headline tensor against the reference's map (golden F11) and a batch of tensors with different seeds."""
    import hashlib
    import json

    import torch
    from tests.inputs import m1_tensor

    f11 = json.loads((golden_dir / "golden_meta_r2.json").read_text())["f11"]["greedy_pcc999_seed123"]
    x = torch.from_numpy(m1_tensor()).to(torch.bfloat16).cuda()
    got = _device_scan_vs_host(x[None], ALL, 0.999, [123])
    assert hashlib.sha256(got[0].reshape(128, 128).tobytes()).hexdigest() == f11["assign_sha256"]
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    xs = (torch.randn((6, 1024, 2048), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    _device_scan_vs_host(xs, ALL, 0.999, [1, 2, 3, 2**31 - 1, 2**40 + 7, 123])
    _device_scan_vs_host(xs, ["bfp8", "bfp4", "bfp2"], 0.995, [5, 6, 7, 8, 9, 10])
    _device_scan_vs_host(xs.float(), ["bfp4", "bfp8", "bf16"], 0.99, [11, 12, 13, 14, 15, 16])     # float32 storage, base bfp4, "upgrades"
    _device_scan_vs_host(xs, ["bf16", "bfp2"], 0.9, [21, 22, 23, 24, 25, 26])
    _device_scan_vs_host(xs[:2], ALL, 0.9999999, [31, 32])                                           # base pass fails: every tile fixed at once
    heavy = (torch.randn((3, 512, 512), generator=g, device="cuda") * 0.02 * torch.exp(1.5 * torch.randn((3, 512, 512), generator=g, device="cuda"))).to(torch.bfloat16)
    for thr in (0.9, 0.99, 0.999, 0.99999):
        _device_scan_vs_host(heavy, ALL, thr, [41, 42, 43])
    small = (torch.randn((4, 32, 128), generator=g, device="cuda") * 0.02).to(torch.bfloat16)           # 4 tiles: shorter than a wave
    _device_scan_vs_host(small, ALL, 0.999, [51, 52, 53, 54])
    _device_scan_vs_host(small[:, :, :32].contiguous(), ALL, 0.999, [61, 62, 63, 64])                   # a single tile


@pytest.mark.gpu
def test_device_scan_large_tensor_global_order():
    """More than 32 768 tiles (Llama-3-8B gate_proj shape: 57 344; and 66 560): the visiting order lives in global scratch instead of LDS."""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = (torch.randn((2, 14336, 4096), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    _device_scan_vs_host(x, ALL, 0.999, [123, 77])
    x = (torch.randn((1, 8192, 8320), generator=g, device="cuda") * 0.02).to(torch.bfloat16)      # 66 560 tiles
    _device_scan_vs_host(x, ALL, 0.999, [5])


@pytest.mark.gpu
def test_device_scan_refusals_and_zero_variance():
    import torch

    x = torch.zeros((2, 64, 128), dtype=torch.bfloat16, device="cuda")           # zero variance: status 1, the host scan is needed
    recs = hb.tile_stats_batched(x, 0xE)
    sd = torch.tensor([5, 6], dtype=torch.int64, device="cuda")
    _maps, status = hb.greedy_scan_device(recs, 0xE | hb.MASK_BF16_IDENTITY, ALL, "pcc", 0.999, 64.0 * 128, sd)
    assert status.cpu().tolist() == [1, 1]
    maps_m, status_m = hb.greedy_scan_device(recs, 0xE | hb.MASK_BF16_IDENTITY, ALL, "mae", 1e-3, 64.0 * 128, sd)   # mae has no denominator: all zeros → every format exact
    assert status_m.cpu().tolist() == [0, 0] and np.array_equal(maps_m.cpu().numpy(), hb.greedy_run_batch(recs.cpu().numpy(), 0xE | hb.MASK_BF16_IDENTITY, ALL, "mae", 1e-3, 64.0 * 128, [5, 6], 1)[0])
    xn = torch.full((1, 64, 128), 0.01, dtype=torch.float32, device="cuda")
    xn[0, 3, 5] = float("nan")                                                    # a NaN maximum: the atol walk hands the tensor to the host scan
    _m, status_n = hb.greedy_scan_device(hb.tile_stats_batched(xn, 0xF), 0xF, ALL, "atol", 1e-3, 64.0 * 128, sd[:1])
    assert status_n.cpu().tolist() == [1]
    with pytest.raises(hb.MtqError):
        hb.greedy_scan_device(recs, 0xE | hb.MASK_BF16_IDENTITY | hb.MASK_SLIM, ALL, "pcc", 0.9, 64.0 * 128, sd)   # full records only
    with pytest.raises(hb.MtqError):
        hb.greedy_scan_device(recs, 0xE | hb.MASK_BF16_IDENTITY, ["bfp8", "bfp8"], "pcc", 0.9, 64.0 * 128, sd)


# ------------------------------------------------------------------------------------------------------------------
# Round 3: partial / listed K1, shared visiting orders, the search in phases
# ------------------------------------------------------------------------------------------------------------------
def _promised_columns(layout, full, sums=0, err=0):
    cols, slot = [], 0
    for f in range(4):
        if not layout & (1 << f):
            continue
        o = 2 + 5 * slot
        if full & (1 << f):
            cols += list(range(o, o + 5))
        elif sums & (1 << f):
            cols += list(range(o, o + 3))
        elif err & (1 << f):
            cols += [o + 3, o + 4]
        slot += 1
    return cols


@pytest.mark.gpu
def test_partial_records_and_listed_completion():
    """mtq_tile_stats_partial writes the promised statistics bit for bit as the whole-record launch does (and NaN elsewhere on the
    exact-integer route); mtq_tile_stats_listed then completes exactly the listed tiles' records — through the four-tiles-per-wave
    exact-integer form (bf16, scratch given), through the one-wave-per-tile form, and by the literal route for the tiles neither
    takes (an Inf, a denormal-only group, a huge exponent)."""
    import torch

    rng = np.random.default_rng(5)
    x = np.stack([gen("normal_bf16", 40 + i, (256, 384)) for i in range(3)])
    x[0, :32, :128] = 0.0                      # an all-zero unit
    x[0, 40, 130] = 3.0e4                      # tail-class neighbours
    x[1, 7, 9] = np.inf                        # the exact routes hand this tile over
    x[2, 64:96, 256:288] = 1e-40               # denormal-only tile
    xd = dev(x, bf16=True)
    count, T = 3, 8 * 12
    for layout, full, sums, lfull, lerr in ((0xE, 0x2, 0x4, 0x8, 0x4), (0x6, 0x0, 0x2, 0x4, 0x2), (0xE, 0x6, 0x0, 0x8, 0x0), (0xC, 0x0, 0x4, 0x8, 0x4)):
        ref = hb.tile_stats_batched(xd, layout)
        got = hb.tile_stats_partial(xd, layout, full, sums)
        cols = [0, 1] + _promised_columns(layout, full, sums)
        assert torch.equal(ref[..., cols].view(torch.int64), got[..., cols].view(torch.int64)), (layout, full, sums)
        # a list with a short last unit, tiles of every tensor, the flagged tiles among them
        ids = np.sort(rng.choice(count * T, size=37, replace=False)).astype(np.int32)
        ids = np.unique(np.concatenate([ids, [T + 0, 2 * T + 2 * 12 + 8]])).astype(np.int32)      # the Inf tile (tensor 1, tile 0) and the denormal tile
        listed = torch.zeros((count * T,), dtype=torch.int32, device="cuda")
        listed[: ids.size] = torch.from_numpy(ids).cuda()
        nl = torch.tensor([ids.size], dtype=torch.int32, device="cuda")
        lcols = _promised_columns(layout, lfull, err=lerr)
        for scratch in (torch.empty((count * T + 1,), dtype=torch.int32, device="cuda"), None):
            work = got.clone()
            hb.tile_stats_listed(xd, layout, lfull, lerr, listed, nl, work, scratch=scratch)
            flat_w, flat_r, flat_g = work.view(count * T, -1), ref.view(count * T, -1), got.view(count * T, -1)
            sel = torch.from_numpy(ids.astype(np.int64)).cuda()
            assert torch.equal(flat_w[sel][:, lcols].view(torch.int64), flat_r[sel][:, lcols].view(torch.int64)), (layout, lfull, lerr, scratch is None)
            rest = torch.ones(count * T, dtype=torch.bool, device="cuda")
            rest[sel] = False
            assert torch.equal(flat_w[rest].view(torch.int64), flat_g[rest].view(torch.int64))              # unlisted tiles untouched
            other = [c for c in range(ref.shape[-1]) if c not in lcols]
            assert torch.equal(flat_w[sel][:, other].view(torch.int64), flat_g[sel][:, other].view(torch.int64))   # nothing else of a listed record touched
    # float32 storage and ragged shapes: every route writes whole records (always allowed), the listed form takes them one wave per tile
    xf = dev(np.stack([gen("heavy_f32", 60 + i, (100, 130)) for i in range(2)]))
    ref = hb.tile_stats_batched(xf, 0xF)
    got = hb.tile_stats_partial(xf, 0xF, 0x3, 0x4)
    cols = [0, 1] + _promised_columns(0xF, 0x3, 0x4)
    assert torch.equal(ref[..., cols].view(torch.int64), got[..., cols].view(torch.int64))
    listed = torch.tensor([1, 5, 19, 20, 39], dtype=torch.int32, device="cuda")
    work = torch.full_like(ref, float("nan"))
    hb.tile_stats_listed(xf, 0xF, 0x8, 0x4, listed, torch.tensor([5], dtype=torch.int32, device="cuda"), work)
    lcols = _promised_columns(0xF, 0x8, err=0x4)
    sel = listed.long()
    assert torch.equal(work.view(40, -1)[sel][:, lcols].view(torch.int64), ref.view(40, -1)[sel][:, lcols].view(torch.int64))
    with pytest.raises(hb.MtqError):
        hb.tile_stats_partial(xd, 0xE, 0x2, 0x2)              # full and sums overlap
    with pytest.raises(hb.MtqError):
        hb.tile_stats_listed(xd, 0xE, 0x1, 0x0, listed, listed[:1], ref)   # bf16 has no late evaluation


@pytest.mark.gpu
def test_scan_orders_are_numpys_permutations():
    """mtq_scan_orders_device: pass 1's and pass 2's orders are what default_rng(seed) hands out after the base pass's permutation —
    in LDS (tiles <= 32 768) and in global memory (above) — and the generator states in between carry on NumPy's stream."""
    import torch

    L = hb.lib()
    for seed, T in ((123, 16384), (7, 1), (7, 2), (2**40 + 9, 4097), (5, 40000)):
        buf = hb.scan_orders_device(seed, T, 2)
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        stride = (T + 63) // 64 * 64
        p = raw[128:128 + 8 * stride].view(np.uint32)
        rng = np.random.default_rng(seed)
        rng.permutation(T)                                    # the base pass's draws
        assert np.array_equal(p[:T], rng.permutation(T).astype(np.uint32)), (seed, T)
        assert np.array_equal(p[stride:stride + T], rng.permutation(T).astype(np.uint32)), (seed, T)
    with pytest.raises(hb.MtqError):
        hb.scan_orders_device(0, 64, 2)
    assert L.mtq_scan_orders_bytes(64) == 128 + 2 * 64 * 4


def _search_variants_vs_host(xs, formats, thr, seed, metric="pcc"):
    """Host scan on whole records = the reference for: the device search with its own shuffles, with the launch's shared orders (helper
    wave), and — pcc, bf16 base, three formats or more — split in phases on partial records with the listed completion in between."""
    import torch

    L = hb.lib()
    count, rows, cols = xs.shape
    ident = xs.dtype == torch.bfloat16 and "bf16" in formats and any(f != "bf16" for f in formats)
    k1 = hb.fmt_mask(formats) & 0xE if ident else hb.fmt_mask(formats)
    dec = k1 | hb.MASK_BF16_IDENTITY if ident else k1
    recs = hb.tile_stats_batched(xs, k1)
    T = recs.shape[1]
    numel = float(rows * cols)
    want, wcounts, _o = hb.greedy_run_batch(recs.cpu().numpy(), dec, formats, metric, thr, numel, [seed] * count, 4)
    sd = torch.full((count,), seed, dtype=torch.int64, device="cuda")
    scratch = torch.empty((int(L.mtq_greedy_scan_scratch_bytes(count, T)),), dtype=torch.uint8, device="cuda")
    maps = torch.empty((count, T), dtype=torch.int8, device="cuda")
    status = torch.empty((count,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((count, 4), dtype=torch.int32, device="cuda")

    def same(tag):
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * count, (tag, formats, thr)
        assert np.array_equal(maps.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), wcounts), (tag, formats, thr, metric)

    hb.greedy_scan_device_ex(recs, dec, formats, metric, thr, numel, sd, maps, status, scratch, counts_out=cnt)
    same("own shuffles")
    orders = hb.scan_orders_device(seed, T, 2)
    maps.fill_(-1)
    hb.greedy_scan_device_ex(recs, dec, formats, metric, thr, numel, sd, maps, status, scratch, counts_out=cnt, orders=orders)
    same("shared orders")
    if len(formats) >= 3 and metric == "pcc" and ident and rows % 32 == 0 and cols % 128 == 0:
        last, prev = hb.fmt_mask([formats[-1]]), hb.fmt_mask([formats[-2]])
        part = hb.tile_stats_partial(xs, k1, k1 & ~last & ~prev, prev)
        listed = torch.empty((count * T,), dtype=torch.int32, device="cuda")
        nl = torch.zeros((1,), dtype=torch.int32, device="cuda")
        carry = torch.empty((int(L.mtq_scan_carry_bytes(count)),), dtype=torch.uint8, device="cuda")
        maps.fill_(-1)
        hb.greedy_scan_device_ex(part, dec, formats, metric, thr, numel, sd, maps, status, scratch, counts_out=cnt, orders=orders, phase=1, listed=listed, n_listed=nl, carry=carry)
        hb.tile_stats_listed(xs, k1, last, prev, listed, nl, part, scratch=torch.empty((count * T + 1,), dtype=torch.int32, device="cuda"))
        hb.greedy_scan_device_ex(part, dec, formats, metric, thr, numel, sd, maps, status, scratch, counts_out=cnt, phase=2, carry=carry)
        same("phases on partial records")
        ns = int(L.mtq_columns_scratch_doubles())
        s_full = torch.empty((count, ns), dtype=torch.float64, device="cuda")
        s_lazy = torch.empty_like(s_full)
        hb.check(L.mtq_column_sums_device_batched(recs.data_ptr(), count, T, dec, maps.data_ptr(), s_full.data_ptr(), hb._stream_ptr()))
        hb.check(L.mtq_column_sums_device_batched(part.data_ptr(), count, T, dec, maps.data_ptr(), s_lazy.data_ptr(), hb._stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(s_full[:, :7].view(torch.int64), s_lazy[:, :7].view(torch.int64)), (formats, thr)   # pcc / mae / atol of the final map
        return int(nl.item())
    return None


@pytest.mark.gpu
def test_device_search_shared_orders_and_phases():
    """Thresholds on both sides of every pass (a pass that accepts everything takes the shared order of the next one; a rejection in
    pass 1 sends the tensor to its own shuffle; a base pass that fails ends the search), format lists of 2–4 entries, the mae metric,
    tensors shorter than a wave, and tensors above 32 768 tiles."""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    xs = (torch.randn((5, 512, 1024), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    listed = {}
    for thr in (0.9, 0.99, 0.999, 0.9999, 0.99999, 0.9999999):
        listed[thr] = _search_variants_vs_host(xs, ALL, thr, 123)
    assert listed[0.9] == 5 * 512 and 0 < listed[0.999] < 5 * 512 and listed[0.9999999] == 0
    _search_variants_vs_host(xs, ["bf16", "bfp8", "bfp4"], 0.999, 7)
    _search_variants_vs_host(xs, ["bf16", "bfp4", "bfp2"], 0.99, 9)
    _search_variants_vs_host(xs, ["bf16", "bfp2", "bfp8", "bfp4"], 0.999, 9)      # an order the partial kernel has no instantiation for: whole slots
    _search_variants_vs_host(xs, ["bf16", "bfp2"], 0.9, 11)
    _search_variants_vs_host(xs, ["bfp8", "bfp4", "bfp2"], 0.995, 5)
    _search_variants_vs_host(xs.float(), ["bfp4", "bfp8", "bf16"], 0.99, 13)
    for thr in (2e-4, 1e-3):
        _search_variants_vs_host(xs, ALL, thr, 31, metric="mae")
    tiny = (torch.randn((4, 32, 128), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    _search_variants_vs_host(tiny, ALL, 0.999, 51)
    _search_variants_vs_host(tiny[:, :, :32].contiguous(), ALL, 0.999, 61)
    heavy = (torch.randn((3, 512, 512), generator=g, device="cuda") * 0.02 * torch.exp(1.5 * torch.randn((3, 512, 512), generator=g, device="cuda"))).to(torch.bfloat16)
    for thr in (0.9, 0.99, 0.999):
        _search_variants_vs_host(heavy, ALL, thr, 41)
    big = (torch.randn((2, 14336, 4096), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    _search_variants_vs_host(big, ALL, 0.999, 123)


@pytest.mark.gpu
def test_lazy_pipeline_equals_whole_record_pipeline(monkeypatch):
    """GreedyPipeline's lazy route (partial K1 → phase 1 → listed K1 → phase 2) and its whole-record route give the same results object
    for object: maps, counts and the three columns bit for bit (both take their column sums from the device in the same tree order);
    seeds at 2^63 and above are seeds too."""
    import torch
    from quantization_analysis_amd.pipeline import GreedyPipeline
    from quantization_analysis_amd.settings import settings

    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    xs = (torch.randn((6, 256, 512), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    xs[1, 32:64, 128:256] *= 1e-28          # groups below the exact route's exponent window: marked by K1, recomputed by the fix-up launch on the search stream
    xs[4, 200, 300] = 2.0e18                # … and one above it (its square still fits float32)
    got = {}
    for lazy in ("1", "0"):
        monkeypatch.setenv("MTQ_LAZY", lazy)
        monkeypatch.setenv("MTQ_K1_TWO_LAUNCH", lazy)   # the whole-record run also takes K1 and its fix-up as one call
        settings(refresh=True)                           # the switches are read once per process (quantization_analysis_amd/settings.py)
        for seeds in (None, [2**63 + 1, 5, 5, 2**64 - 1, 9, 123]):
            with GreedyPipeline(ALL, "pcc", 0.999, 2**63 + 12345, chunk=4, workers=2) as pipe:
                assert (pipe.lazy_plan(xs) is not None) == (lazy == "1")
                res = pipe.run(xs, seeds=seeds)
                got[(lazy, seeds is None)] = res
                if lazy == "1":
                    assert pipe.listed_tiles > 0
    for key in (True, False):
        for a, b in zip(got[("1", key)], got[("0", key)]):
            assert np.array_equal(a.assignment, b.assignment) and a.counts == b.counts
            assert np.array_equal(np.array([a.pcc, a.mae, a.atol]).view(np.uint64), np.array([b.pcc, b.mae, b.atol]).view(np.uint64))
    x0 = xs[0].float().cpu().numpy()
    a, counts, _st = orc.greedy(x0, ALL, "pcc", 0.999, 2**63 + 12345)
    assert np.array_equal(got[("1", True)][0].assignment, a) and got[("1", True)][0].counts == counts
    # a threshold most tiles pass down to the last format: the first batch lists nearly every tile, and the route switches itself off for that
    # tile count — same results from the lazy batch, the whole-record batches after it and the oracle
    monkeypatch.setenv("MTQ_LAZY", "1")
    settings(refresh=True)
    with GreedyPipeline(ALL, "pcc", 0.9, 77, chunk=6, workers=2) as pipe:
        assert pipe.lazy_plan(xs) is not None
        first = pipe.run(xs)
        assert pipe.lazy_off and pipe.lazy_plan(xs) is None and pipe.lazy_plan(xs[:, :128]) is not None
        second = pipe.run(xs)
    for r1, r2 in zip(first, second):
        assert np.array_equal(r1.assignment, r2.assignment) and r1.counts == r2.counts and (r1.pcc, r1.mae, r1.atol) == (r2.pcc, r2.mae, r2.atol)
    a, counts, _st = orc.greedy(x0, ALL, "pcc", 0.9, 77)
    assert np.array_equal(first[0].assignment, a) and first[0].counts == counts


def test_pipeline_under_force_generic_switch():
    """MTQ_FORCE_GENERIC=1 (the A/B switch that sends every K1 through the literal kernel; read once per process by the library, hence a
    subprocess): GreedyPipeline must not take the two-launch form the exact kernel's entry point refuses then — same maps as the oracle; and a
    ragged batch goes through the literal kernel with its table — the records of the per-matrix calls."""
    import os
    import subprocess
    import sys

    code = (
        "import numpy as np, torch\n"
        "from oracle import mtq_oracle as orc\n"
        "from quantization_analysis_amd.pipeline import GreedyPipeline\n"
        "from tests.inputs import gen\n"
        "xs = np.stack([gen('normal_bf16', 40 + i, (64, 256)) for i in range(3)])\n"
        "x = torch.from_numpy(xs).cuda().to(torch.bfloat16)\n"
        "with GreedyPipeline(['bf16', 'bfp8', 'bfp4', 'bfp2'], 'pcc', 0.999, 123, chunk=2, workers=2) as pipe:\n"
        "    res = pipe.run(x)\n"
        "for i, r in enumerate(res):\n"
        "    a, c, _ = orc.greedy(xs[i], ['bf16', 'bfp8', 'bfp4', 'bfp2'], 'pcc', 0.999, 123)\n"
        "    assert np.array_equal(r.assignment, a) and r.counts == c, i\n"
        "from quantization_analysis_amd import hip_backend as hb\n"
        "ms = [torch.from_numpy(gen('heavy_f32', 60 + i, sh)).cuda() for i, sh in enumerate([(70, 100), (32, 32), (64, 40)])]\n"
        "got = hb.tile_stats_ragged(ms, 0xF).cpu().numpy().view(np.int64)\n"
        "want = np.concatenate([hb.tile_stats(m, 0xF).cpu().numpy().view(np.int64) for m in ms])\n"
        "assert np.array_equal(got, want)\n"
        "print('ok')\n")
    env = dict(os.environ, MTQ_FORCE_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=str(Path(__file__).resolve().parent.parent))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
