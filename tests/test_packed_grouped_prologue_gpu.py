"""GPU: the grouped skinny entries with the X prologue inside the kernel (prologue="fused" on glu_grouped_skinny, linear_grouped, moe_glu,
moe_down_combine and PackedMoE): bit for bit the float64 reference of tests/grouped_prologue_cases.py on its exact inputs - 3 experts of
96 x 2048 with 0, 1 and 33 rows, so an empty expert, a one-row chunk, a full chunk and a wave without a tile row that keeps the barriers -
and bit for bit the staged route on random inputs with an Inf, a NaN and a value the shift makes subnormal."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb, packed
from tests import grouped_prologue_cases as cases

pytestmark = pytest.mark.gpu


def bits(y):
    return y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16)


@pytest.mark.parametrize("split", (0, 1, 2))   # block 1024: two panels per slice at split 1, one at split 2
@pytest.mark.parametrize("block,shifts", cases.CASES)
@pytest.mark.parametrize("entry", cases.ENTRIES)
def test_fused_is_the_float64_reference(entry, block, shifts, split):
    torch.cuda.set_device(0)
    for mixed in (False, True):
        got, want = cases.run(entry, block, shifts, mixed, "hip", "fused", split)
        assert np.array_equal(got, want) and np.abs(want).max() > 0, mixed


def experts(rng, count, n, k):
    """Gaussian experts under random maps, packed on the device (bit equality of two routes asks nothing more of the weights)."""
    w = torch.from_numpy(rng.standard_normal((count, n, k)).astype(np.float32)).cuda()
    return packed.as_batch(packed.pack_batch(w, rng.integers(0, 4, (count, n // 32, k // 32)).astype(np.int8), backend="hip"))


@pytest.mark.parametrize("block", (0, 32, 128))
def test_fused_equals_staged_bit_for_bit(block):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(block)
    count, n, k = cases.COUNT, cases.N, cases.K
    p = rng.integers(0, 8, (count, k))
    p[2, 7] = 7
    gate, up, down = (experts(rng, count, n, k) for _ in range(3))
    x = torch.from_numpy(rng.standard_t(3, (36, k)).astype(np.float32)).to(torch.bfloat16)
    x[0, 3], x[1, 5], x[2, 7] = float("inf"), float("nan"), 2.0 ** -126   # row 2 is expert 2's: 2^-126 · 2^-7 is subnormal
    x = x.cuda()
    eff = hb.packed_grouped_pre_split(count, 34, n, k, block)
    g = torch.from_numpy(cases.GROUP_ROWS.astype(np.int32)).cuda()
    kw = dict(rotate=block, in_exponents=p)
    for out_dtype in ("float32", "bfloat16"):
        want = packed.glu_grouped_skinny(x[:34], g, gate, up, out_dtype=out_dtype, split=eff, prologue="staged", **kw)
        assert torch.equal(bits(packed.glu_grouped_skinny(x[:34], g, gate, up, out_dtype=out_dtype, prologue="fused", **kw)), bits(want))
        want = packed.linear_grouped(x[:34], g, down, out_dtype=out_dtype, split=eff, prologue="staged", **kw)
        assert torch.equal(bits(packed.linear_grouped(x[:34], g, down, out_dtype=out_dtype, prologue="fused", **kw)), bits(want))
        plan = packed.moe_plan(torch.tensor(cases.DOWN_IDS).cuda(), count)
        weights = torch.from_numpy(rng.random((18, 2)).astype(np.float32)).cuda()
        for expert_dtype in ("float32", "bfloat16"):
            more = dict(expert_dtype=expert_dtype, out_dtype=out_dtype, **kw)
            want = packed.moe_down_combine(x, weights, plan, down, split=hb.packed_grouped_pre_split(count, 36, n, k, block), prologue="staged", **more)
            assert torch.equal(bits(packed.moe_down_combine(x, weights, plan, down, prologue="fused", **more)), bits(want))
        plan = packed.moe_plan(torch.tensor(cases.GLU_IDS).cuda(), count)
        want = packed.moe_glu(x[:5], plan, gate, up, out_dtype=out_dtype, split=hb.packed_grouped_pre_split(count, 10, n, k, block),
                              prologue="staged", **kw)
        assert torch.equal(bits(packed.moe_glu(x[:5], plan, gate, up, out_dtype=out_dtype, prologue="fused", **kw)), bits(want))


@pytest.mark.parametrize("decode_route", packed.MOE_DECODE_ROUTES)
def test_packed_moe_fused_equals_staged(decode_route):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(5)
    count, k, hidden = 8, 1024, 2048               # shapes at which the fused and the unfused rule choose one split (4 and 16)
    assert hb.packed_grouped_pre_split(count, 10, hidden, k, 256) == hb.packed_grouped_pre_split(count, 10, hidden, k, 0) == 4
    assert hb.packed_grouped_pre_split(count, 10, 96, hidden, 64) == hb.packed_grouped_pre_split(count, 10, 96, hidden, 0) == 16
    p, pd = rng.integers(0, 8, (count, k)), rng.integers(0, 8, (count, hidden))
    gate, up, down = experts(rng, count, hidden, k), experts(rng, count, hidden, k), experts(rng, count, 96, hidden)
    x = torch.from_numpy(rng.standard_t(3, (5, k)).astype(np.float32)).to(torch.bfloat16).cuda()
    ids = torch.from_numpy(rng.integers(0, count + 1, (5, 2))).cuda()           # an id of `count` is dropped
    w = torch.from_numpy(rng.random((5, 2)).astype(np.float32)).cuda()
    kw = dict(decode_max_rows=64, decode_route=decode_route)
    pre = dict(rotate=256, in_exponents=p, down_rotate=64, down_in_exponents=pd)
    fused, staged = (packed.PackedMoE(gate, up, down, prologue=pr, **pre, **kw)(x, ids, w) for pr in ("fused", "staged"))
    assert torch.equal(bits(fused), bits(staged)) and bool(fused.float().abs().max() > 0)
    plain = packed.PackedMoE(gate, up, down, **kw)(x, ids, w)                 # the defaults: today's module, whatever `prologue` says
    assert torch.equal(bits(packed.PackedMoE(gate, up, down, prologue="fused", **kw)(x, ids, w)), bits(plain))
    plan = packed.moe_plan(ids, count)
    today = packed.moe_down_combine(packed.moe_glu(x, plan, gate, up), w, plan, down, out_dtype="bfloat16")
    assert torch.equal(bits(plain), bits(today)) and not torch.equal(bits(plain), bits(fused))
