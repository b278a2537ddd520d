"""CPU-only: include/mtq_grouped_pre.h against GROUPED_PRE_SIGNATURES, the refusals and the split rule of the *_grouped_pre entries that
need no device, the staged emulation route of the four grouped entries against the plain float64 reference of
tests/grouped_prologue_cases.py (every row), and what prologue="fused" refuses without a device."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb, packed
from tests import grouped_prologue_cases as cases

LETTER = {"int": "i", "int64_t": "l", "size_t": "z"}


def test_header_is_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).parents[1] / "include" / "mtq_grouped_pre.h").read_text(), flags=re.S)
    found = {}
    for result, name, params in re.findall(r"^(int|size_t) (mtq_\w+)\(([^;]*)\);", text, flags=re.M):
        kinds = ["p" if "*" in p else LETTER[p.split()[0]] for p in params.replace("\n", " ").split(",")]
        found[name] = (LETTER[result], "".join(kinds), True)
    assert found == hb.GROUPED_PRE_SIGNATURES and hb.grouped_pre_available()


HOST = 4096   # a host address no check may dereference


def glu_args(k=2048, block=64, exps=None, split=1):
    return (HOST, 34, 1, k, k, None, HOST, block, exps, *(HOST, 1 << 22, HOST, HOST, HOST) * 2, 3, 96, None, None, 0, 0, HOST, hb.DTYPE_F32, 96,
            split, HOST, 1 << 24, None)


def linear_args(k=2048, block=64, exps=None, split=1):
    return (HOST, k, k, HOST, block, exps, HOST, 1 << 22, HOST, HOST, HOST, 3, 96, hb.DTYPE_F32, None, None, 0, None, 0, 0, 34, 1, HOST,
            hb.DTYPE_F32, 96, split, HOST, 1 << 24, None)


@pytest.mark.parametrize("kw,text", (
    (dict(block=48), "power of two"), (dict(block=2048), "1024"), (dict(k=2080), "multiple of block"), (dict(split=3), "equal slices"),
    (dict(block=1024, split=4), "equal slices"), (dict(block=0), "no prologue"), (dict(exps=HOST + 4), "in_exponents must be 16-byte aligned")))
@pytest.mark.parametrize("entry,args", (("mtq_packed_glu_skinny_grouped_pre", glu_args), ("mtq_packed_linear_skinny_grouped_pre", linear_args)))
def test_refusals_without_a_device(entry, args, kw, text):
    assert hb._entry(entry)(*args(**kw)) == -1
    assert text in hb.lib().mtq_last_error().decode()


@pytest.mark.parametrize("count,n,k,block,split,want", (
    (3, 96, 2048, 0, 0, 16), (3, 96, 2048, 64, 0, 16), (3, 96, 2048, 1024, 0, 2), (3, 96, 2048, 256, 2, 2), (3, 96, 3072, 1024, 0, 3),
    (256, 2048, 7168, 256, 0, 1), (8, 4096, 4096, 256, 0, 2), (3, 96, 2048, 0, 5, 5)))
def test_split_rule(count, n, k, block, split, want):
    assert hb.packed_grouped_pre_split(count, 34, n, k, block, split) == want
    assert hb.packed_glu_skinny_grouped_pre_workspace(34, count, n, k, block, split) == hb.packed_glu_skinny_grouped_workspace_bytes(34, count, n, k, want)
    assert hb.packed_linear_skinny_grouped_pre_workspace(34, count, n, k, block, split) == \
        hb.packed_linear_skinny_grouped_workspace_bytes(34, count, n, k, want)
    assert hb.packed_linear_skinny_grouped_pre_workspace(34, count, n, k, block, split, combine=True) == \
        hb.moe_down_combine_workspace_bytes(34, count, n, k, want)


@pytest.mark.parametrize("mixed", (False, True))
@pytest.mark.parametrize("block,shifts", cases.CASES)
@pytest.mark.parametrize("entry", cases.ENTRIES)
def test_staged_emulation_is_the_float64_reference(entry, block, shifts, mixed):
    got, want = cases.run(entry, block, shifts, mixed, "emulation", "staged")
    assert np.array_equal(got, want) and np.abs(want).max() > 0


def test_fused_refused_with_its_reason():
    (gate, _), (up, _) = cases.experts(1, False, "emulation"), cases.experts(2, False, "emulation")
    x = cases.exact_x(np.random.default_rng(0), 34, 64)
    for kw, why in ((dict(), "emulation"), (dict(kernel="chunks"), "chunks")):
        with pytest.raises(hb.MtqError, match=why):
            packed.glu_grouped_skinny(x, cases.GROUP_ROWS, gate, up, rotate=64, prologue="fused", backend="emulation", **kw)
        with pytest.raises(hb.MtqError, match=why):
            packed.linear_grouped(x, cases.GROUP_ROWS, gate, rotate=64, prologue="fused", backend="emulation", **kw)
    plan = packed.moe_plan(torch.tensor(cases.GLU_IDS), cases.COUNT)
    with pytest.raises(hb.MtqError, match="transpose"):
        packed.moe_glu(x[:5, :96], plan, gate, up, stored="transpose", rotate=32, prologue="fused")
    down = packed.pack_batch(np.zeros((cases.COUNT, 32, cases.N), dtype=np.float32), np.zeros((cases.COUNT, 1, 3), dtype=np.int8))
    with pytest.raises(hb.MtqError, match="emulation"):
        packed.PackedMoE(gate, up, down, backend="emulation", decode_max_rows=64, rotate=64, prologue="fused")
    with pytest.raises(hb.MtqError, match="prologue must be one of"):
        packed.PackedExpertsMLP(gate, up, down, prologue="fast")
