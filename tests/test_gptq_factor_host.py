"""mtq_gptq_factor without a GPU: argument checks before a device is looked for, the exported block size, the emulation's refusal."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.layer_io import select_ops
from quantization_analysis_amd.model_source import build_model_index
from quantization_analysis_amd.output_error import evaluate_op
from tests.test_output_error_host import make_fixture


def test_block_size_is_the_headers():
    m = re.search(r"#define\s+MTQ_GPTQ_FACTOR_BLOCK\s+(\d+)", (Path(__file__).resolve().parent.parent / "include" / "mtq.h").read_text())
    assert m and int(m.group(1)) == hb.GPTQ_FACTOR_BLOCK


def test_c_entry_checks_arguments_before_a_device():
    L, nb = hb.lib(), hb.GPTQ_FACTOR_BLOCK
    size = L.mtq_gptq_factor_scratch_doubles
    assert size(0) == 0 and size(-3) == 0 and size(1) == size(nb) == 3 * nb * nb and size(nb + 1) == 8 * nb * nb
    k = 40
    buf = np.zeros(size(k) + 2, dtype=np.float64)
    p = buf.ctypes.data
    p += p % 16                                                 # numpy aligns to 8 at least
    ok = dict(hd=p, k=k, u=p, ud=k * k, status=p, s=p, sd=size(k), st=None)

    def call(**kw):
        return L.mtq_gptq_factor(*{**ok, **kw}.values())

    for key in ("hd", "u", "status", "s"):
        assert call(**{key: None}) == -1 and b"null" in L.mtq_last_error()
    assert call(k=0) == -1 and call(k=-1) == -1
    assert call(k=(1 << 17) + 1, ud=((1 << 17) + 1) ** 2) == -1 and b"too large" in L.mtq_last_error()
    assert call(ud=k * k - 1) == -1 and b"u_doubles" in L.mtq_last_error()
    assert call(sd=size(k) - 1) == -1 and b"scratch" in L.mtq_last_error()
    assert call(s=p + 8) == -1 and b"aligned" in L.mtq_last_error()
    if not torch.cuda.is_available():
        assert call() == -3                                     # every argument passes: only the device is missing


def test_device_factor_is_refused_on_the_emulation_backend(tmp_path):
    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp.down_proj", "test")
    for factor in ("device", "gpu"):
        with pytest.raises(ValueError, match="factor"):
            evaluate_op(index, ops[0], ["bfp4"], None, "emulation", calib=None, gptq=True, gptq_factor=factor)
