"""GPU: the skinny entries with the X prologue inside (packed.linear / glu_skinny / PackedLinear / PackedMLP with prologue="fused"):
bit equality with the staged route hadamard → ldexp → skinny at the same split, exact float64 agreement on integer data, the refusals
and "auto", and PackedMLP against its staged form and the emulation."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import awq, hadamard as hd, hip_backend as hb, packed

pytestmark = pytest.mark.gpu
SHAPES = ((96, 2048), (80, 3072))   # three tile rows (one wave of the workgroup has no unit); a ragged tile row
BLOCKS = (0, 32, 64, 256, 1024)


def own_split(n, k, B):
    """The fused rule: the largest s <= the skinny rule's with equal slices of whole blocks."""
    th, tw, bt = -(-n // 32), k // 32, max(B // 32, 1)
    return max(s for s in range(1, max(1, min(2048 // th, tw // 4)) + 1) if B == 0 or (tw % s == 0 and tw // s % bt == 0))


def splits(n, k, B):
    """1, 2 and the rule's own, without the pairs the slice rule refuses."""
    return sorted({s for s in (1, 2, own_split(n, k, B)) if B == 0 or (k // 32 % s == 0 and k // 32 // s % (B // 32) == 0)})


def deployed(rng, n, k, B, p, codes, backend="hip"):
    """A Gaussian weight rotated and scaled as deployment does, packed under `codes` (one format, or None: all four)."""
    w = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32))
    w = hd.rotate_weight(w, B) if B else w
    w = awq.scale_weight(w, p) if p is not None else w
    amap = rng.integers(0, 4, (-(-n // 32), k // 32)) if codes is None else np.full((-(-n // 32), k // 32), codes)
    return packed.pack(w.cuda() if backend == "hip" else w, amap, backend=backend)


def staged_x(x, B, p):
    x = hd.hadamard(x, B, out_dtype=torch.bfloat16, backend="hip") if B else x
    return x if p is None else torch.ldexp(x, -torch.from_numpy(p.astype(np.int32)).cuda())


def bits(y):
    return y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_linear_fused_equals_staged_bit_for_bit(n, k, B):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + B)
    bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    wide = torch.from_numpy(rng.standard_t(3, (32, k + 24)).astype(np.float32)).to(torch.bfloat16).cuda()
    xs = {m: wide[:m, :k].contiguous() for m in (1, 5, 32)}
    xs["view"] = wide.reshape(-1)[3:3 + 5 * (k + 24)].reshape(5, k + 24)[:, :k]   # padded ldx and an odd element offset: no 16-byte loads
    for p in (None, rng.integers(0, 8, k)):
        if B == 0 and p is None:
            continue
        for codes in (None, 2):
            pt = deployed(rng, n, k, B, p, codes)
            for x in xs.values():
                want_x = staged_x(x, B, p)
                for s in splits(n, k, B):
                    for out_dtype in ("float32", "bfloat16"):
                        want = packed.linear(want_x, pt, bias=bias, out_dtype=out_dtype, kernel="skinny", split=s)
                        got = packed.linear(x, pt, bias=bias, out_dtype=out_dtype, rotate=B, in_exponents=p, prologue="fused", split=s)
                        assert torch.equal(bits(got), bits(want)), (x.shape[0], p is not None, codes, s, out_dtype)


@pytest.mark.parametrize("B", (0, 64))
@pytest.mark.parametrize("n,k", SHAPES)
def test_glu_skinny_fused_equals_staged_bit_for_bit(n, k, B):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + B + 1)
    for p in (None, rng.integers(0, 8, k)):
        if B == 0 and p is None:
            continue
        gate, up = deployed(rng, n, k, B, p, None), deployed(rng, n, k, B, p, None)
        for m in (1, 32):
            x = torch.from_numpy(rng.standard_t(3, (m, k)).astype(np.float32)).to(torch.bfloat16).cuda()
            for s in splits(n, k, B):
                for out_dtype in ("float32", "bfloat16"):
                    want = packed.glu_skinny(staged_x(x, B, p), gate, up, act="silu", out_dtype=out_dtype, split=s)
                    got = packed.glu_skinny(x, gate, up, act="silu", out_dtype=out_dtype, split=s, rotate=B, in_exponents=p, prologue="fused")
                    assert torch.equal(bits(got), bits(want)), (m, p is not None, s, out_dtype)


@pytest.mark.parametrize("codes", (0, 1))
@pytest.mark.parametrize("B", (64, 256, 1024))
def test_fused_linear_is_exact_on_integer_data(B, codes):
    """Integer X in [-8, 8], W in {-1, 0, 1} (its own value under bf16 and bfp8), p in 0 .. 7, k = 2048.  X″ is a multiple of
    2^-(log2(B)/2 + 7) >= 2^-12, and sum_k |X″||W| of every output stays below 2^24 of those units (asserted below on the data: about
    2^22.4 at B = 1024), so every partial sum in any order is exact in float32 and the result equals the float64 product exactly."""
    torch.cuda.set_device(0)
    rng = np.random.default_rng(B + codes)
    m, n, k = 5, 96, 2048
    x = torch.from_numpy(rng.integers(-8, 9, (m, k)).astype(np.float32)).to(torch.bfloat16)
    w, p = rng.integers(-1, 2, (n, k)).astype(np.float32), rng.integers(0, 8, k)
    b = rng.integers(-4, 5, n).astype(np.float32)
    x2 = np.ldexp(hd.hadamard_emulation(x, B, torch.bfloat16).double().numpy(), -p)
    assert (np.abs(x2) @ np.abs(w.astype(np.float64)).T).max() * 2.0 ** (int(np.log2(B)) // 2 + 7) < 2 ** 24
    pt = packed.pack(torch.from_numpy(w).cuda(), np.full((n // 32, k // 32), codes), backend="hip")
    got = packed.linear(x.cuda(), pt, bias=torch.from_numpy(b).cuda(), rotate=B, in_exponents=p, prologue="fused")
    assert np.array_equal(got.cpu().numpy().astype(np.float64), x2 @ w.astype(np.float64).T + b)


def test_refusals_auto_and_defaults(monkeypatch):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    n, k, B = 96, 3072, 1024
    pt = deployed(rng, n, k, B, None, None)
    x = torch.from_numpy(rng.standard_t(3, (33, k)).astype(np.float32)).to(torch.bfloat16).cuda()
    for xm, s in ((x[:5], 2), (x, 0)):                  # a slice of 1.5 blocks; m = 33
        with pytest.raises(hb.MtqError):
            packed.linear(xm, pt, rotate=B, prologue="fused", kernel="auto", split=s)
        want = packed.linear(staged_x(xm, B, None), pt, kernel="auto", split=s)
        assert torch.equal(bits(packed.linear(xm, pt, rotate=B, prologue="auto", kernel="auto", split=s)), bits(want))
    for kernel in ("block", "skinny"):                  # the defaults are today's calls
        assert torch.equal(bits(packed.linear(x[:5], pt, kernel=kernel, prologue="staged")), bits(packed.linear(x[:5], pt, kernel=kernel)))
    assert torch.equal(packed.PackedLinear(pt, rotate=B)(x[:5]), packed.linear(staged_x(x[:5], B, None), pt, kernel="auto"))
    calls, entry = [], hb.packed_linear_skinny_pre     # in its measured range "auto" is the fused entry, from the function and the module
    monkeypatch.setattr(hb, "packed_linear_skinny_pre", lambda *a, **kw: calls.append(kw["block"]) or entry(*a, **kw))
    want = packed.linear(x[:5], pt, rotate=B, prologue="fused", split=1)
    assert torch.equal(bits(packed.linear(x[:5], pt, rotate=B, prologue="auto", kernel="auto", split=1)), bits(want))
    assert torch.equal(bits(packed.PackedLinear(pt, rotate=B, prologue="auto")(x[:5])), bits(packed.linear(x[:5], pt, rotate=B, prologue="fused")))
    assert calls == [B] * 4


def exact_bits(a, w):
    """log2 of the largest sum_k |a||w| of an output in units of the lowest set bit among its terms: below 24, every partial sum of the
    product a @ w.T, in any order, is exact in float32."""
    mant, e = np.frexp(np.abs(a))
    i = (mant * 2.0 ** 53).astype(np.int64)
    low = np.where(a != 0, np.ldexp((i & -i).astype(np.float64), e - 53), np.inf)
    unit = np.where(w[None] != 0, low[:, None, :], np.inf).min(-1)
    return float(np.log2((np.abs(a) @ np.abs(w).T / unit).max()))


def test_packed_mlp_fused_prologue():
    """128 -> 256 -> 96 at m = 4, both halves through the _pre entries: the staged module's bits, and the emulation module's value
    EXACTLY on exact-arithmetic inputs: integer X in [-8, 8], shifts in 0 .. 7, W in {-1, 0, 1} under bf16 and bfp8 maps (the down
    weight one in sixteen nonzero), act="none", blocks of 64.  g and u are exact in float32 (below 2^17 units, asserted), g * u is rounded
    once to float32 and from there to bf16 on both backends, the rotation of h is the same float32 butterflies, and every partial sum
    of the down projection is exact (below 2^24 units of its lowest term bit, asserted on the data: 2^19.1)."""
    torch.cuda.set_device(0)
    rng = np.random.default_rng(2)
    k, hidden, out, m = 128, 256, 96, 4
    p = rng.integers(0, 8, k)
    x = torch.from_numpy(rng.integers(-8, 9, (m, k)).astype(np.float32)).to(torch.bfloat16)
    ws = [rng.integers(-1, 2, (hidden, k)).astype(np.float32) for _ in range(2)]
    ws.append((rng.integers(-1, 2, (out, hidden)) * (rng.random((out, hidden)) < 0.0625)).astype(np.float32))
    x2 = np.ldexp(hd.hadamard_emulation(x, 64, torch.bfloat16).double().numpy(), -p)
    h = torch.from_numpy((x2 @ ws[0].T) * (x2 @ ws[1].T)).float().to(torch.bfloat16)
    h2 = hd.hadamard_emulation(h, 64, torch.bfloat16).double().numpy()
    assert max(exact_bits(x2, ws[0]), exact_bits(x2, ws[1])) < 17 and exact_bits(h2, ws[2]) < 24
    maps = [np.full((w.shape[0] // 32, w.shape[1] // 32), c) for w, c in zip(ws, (0, 1, 1))]
    dev = [packed.pack(torch.from_numpy(w).cuda(), a, backend="hip") for w, a in zip(ws, maps)]
    host = [packed.pack(torch.from_numpy(w), a, backend="emulation") for w, a in zip(ws, maps)]
    kw = dict(act="none", rotate=64, in_exponents=p, down_rotate=64, decode_kernel="fused", out_dtype="float32")
    got = packed.PackedMLP(*dev, prologue="fused", **kw)(x.cuda())
    assert torch.equal(bits(got), bits(packed.PackedMLP(*dev, prologue="staged", **kw)(x.cuda())))
    assert np.array_equal(got.cpu().numpy(), packed.PackedMLP(*host, backend="emulation", **kw)(x).numpy())
    assert np.array_equal(got.cpu().numpy().astype(np.float64), h2 @ ws[2].astype(np.float64).T)
