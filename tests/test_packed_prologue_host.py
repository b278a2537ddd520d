"""CPU-only: the fused prologue's split rule against the exported C function, the emulation backend's prologue arguments against the
explicit composition, and the refusals that need no device."""
import numpy as np
import pytest
import torch

from quantization_analysis_amd import awq, hadamard as hd, hip_backend as hb, packed


@pytest.mark.parametrize("B", (0, 32, 256, 1024))
@pytest.mark.parametrize("n,k", ((96, 2048), (80, 3072), (4096, 4096), (14336, 4096), (4096, 14336), (32, 1024)))
def test_split_rule(n, k, B):
    th, tw, bt = -(-n // 32), k // 32, max(B // 32, 1)
    skinny = max(1, min(2048 // th, tw // 4))
    want = max(s for s in range(1, skinny + 1) if B == 0 or (tw % s == 0 and tw // s % bt == 0))
    assert hb.packed_skinny_pre_split(5, n, k, B) == want
    assert hb.packed_linear_skinny_pre_workspace(5, n, k, B) == hb.packed_linear_skinny_workspace_bytes(5, n, k, want)
    assert hb.packed_glu_skinny_pre_workspace(5, n, k, B) == hb.packed_glu_skinny_workspace_bytes(5, n, k, want)


def test_refusals_without_a_device():
    for m, n, k, B, s in ((5, 96, 3072, 1024, 2), (33, 96, 2048, 64, 0), (5, 96, 4096, 2048, 0), (5, 96, 2048, 48, 0), (5, 96, 2080, 64, 0)):
        with pytest.raises(hb.MtqError):
            hb.packed_skinny_pre_split(m, n, k, B, s)
    fn, host = hb._entry("mtq_packed_linear_skinny_pre"), 4096     # host addresses no check may dereference
    assert fn(host, 5, 2048, 2048, 0, None, host, 1 << 20, host, host, 96, None, host, hb.DTYPE_F32, 96, 1, None, 0, None) != 0
    assert "nothing" in hb.lib().mtq_last_error().decode() or "no prologue" in hb.lib().mtq_last_error().decode()
    assert fn(host, 5, 2048, 2048, 64, 4100, host, 1 << 20, host, host, 96, None, host, hb.DTYPE_F32, 96, 1, None, 0, None) != 0
    assert "in_exponents must be 16-byte aligned" in hb.lib().mtq_last_error().decode()


@pytest.mark.parametrize("prologue", ("staged", "auto"))
def test_emulation_prologue_is_the_composition(prologue):
    rng = np.random.default_rng(3)
    n, k, B = 64, 256, 64
    p = rng.integers(0, 8, k)
    w = awq.scale_weight(hd.rotate_weight(torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32)), B), p)
    pt = packed.pack(w, rng.integers(0, 4, (n // 32, k // 32)), backend="emulation")
    x = torch.from_numpy(rng.standard_t(3, (5, k)).astype(np.float32)).to(torch.bfloat16)
    x2 = torch.ldexp(hd.hadamard_emulation(x, B, torch.bfloat16), -torch.from_numpy(p.astype(np.int32)))
    want = packed.linear(x2, pt, backend="emulation")
    assert np.array_equal(packed.linear(x, pt, backend="emulation", rotate=B, in_exponents=p, prologue=prologue), want)
    assert np.array_equal(packed.PackedLinear(pt, backend="emulation", rotate=B, in_exponents=p, prologue=prologue)(x).numpy(), want)
    with pytest.raises(hb.MtqError, match="emulation"):
        packed.linear(x, pt, backend="emulation", rotate=B, in_exponents=p, prologue="fused")
    with pytest.raises(hb.MtqError, match="prologue must be one of"):
        packed.PackedMLP(pt, pt, pt, prologue="fast")
