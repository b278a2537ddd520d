"""CPU-only: the `transpose` algorithm — registration, the emulation results against the reference's (F15), the cache rule, `wq`
with the example config, and the argument checks of the two transposed entry points (C ABI and binding) without a GPU."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms import ALGORITHM_REGISTRY, LAYOUT_ALGORITHMS, create_algorithm
from quantization_analysis_amd.compression_algorithms.cache import CacheContext
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from quantization_analysis_amd.compression_algorithms.transpose import TransposeCompression

ROOT = Path(__file__).resolve().parent.parent
FORMATS = ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
CONFIG = ROOT / "compression_configs" / "compression_config.transpose.example.json"


@pytest.fixture(scope="module")
def f15(golden_dir):
    return np.load(golden_dir / "f15_transpose.npz"), json.loads((golden_dir / "golden_meta_f15.json").read_text())


def _cache(tmp_path, recompute=True):
    return CacheContext(root=tmp_path, tensor_name="t", backend="emulation", recompute=recompute, run_tag="test")


def test_registry():
    assert set(ALGORITHM_REGISTRY) == {"none", "mixed-tile-greedy", "mixed-tile-threshold", "mixed-tile", "mixed-tile-random"}
    assert LAYOUT_ALGORITHMS == {"transpose": TransposeCompression}
    a = create_algorithm(" Transpose ", {})
    assert isinstance(a, TransposeCompression) and a.name == "transpose"
    with pytest.raises(ValueError, match="Supported: .*transpose"):
        create_algorithm("nope")


def test_emulation_equals_reference(f15, tmp_path):
    data, meta = f15
    for case in meta["cases"]:
        x = data[f"{case}__x"]
        res = create_algorithm("transpose").run(x, FORMATS, Quantizer("emulation"), _cache(tmp_path))
        assert [r.fmt for r in res] == [f.upper() for f in FORMATS]
        assert all(r.compression == "transpose" and r.tile_counts is None and r.meta is None for r in res)
        for fmt, r in zip(FORMATS, res):
            y = np.asarray(r.y, dtype=np.float32)
            assert y.shape == x.shape, (case, fmt)
            assert np.array_equal(np.ascontiguousarray(y).view(np.uint32), data[f"{case}__{fmt}"]), (case, fmt)


def test_identity_through_a_2d_view(f15):
    """quantize(V.T).T with V = x.reshape(x.shape[0], -1) is the reference's result for every rank (the route the hip backend takes)."""
    from quantization_analysis_amd.quantization_formats import quantize_weight_values

    data, meta = f15
    for case in meta["cases"]:
        x = data[f"{case}__x"]
        d0 = x.shape[0] if x.ndim else 1
        v = x.reshape(d0, -1)
        for fmt in FORMATS:
            with np.errstate(all="ignore"):
                y = quantize_weight_values(np.ascontiguousarray(v.T), fmt).T.reshape(x.shape)
            assert np.array_equal(np.ascontiguousarray(y, dtype=np.float32).view(np.uint32), data[f"{case}__{fmt}"]), (case, fmt)


def test_cache_reuse_and_shape_rule(tmp_path):
    x = (np.random.default_rng(3).standard_normal((40, 24)) * 0.02).astype(np.float32)
    algo = create_algorithm("transpose")
    first = algo.run(x, ["bfp4"], Quantizer("emulation"), _cache(tmp_path, recompute=False))[0].y
    path = _cache(tmp_path).quant_path("transpose", "bfp4")
    assert path.exists()
    marked = np.full_like(first, 7.0)
    np.save(path, marked)
    again = algo.run(x, ["bfp4"], Quantizer("emulation"), _cache(tmp_path, recompute=False))[0].y
    assert np.array_equal(again, marked)                                  # same shape: the cached y is used
    np.save(path, np.zeros((3, 3), dtype=np.float32))
    fresh = algo.run(x, ["bfp4"], Quantizer("emulation"), _cache(tmp_path, recompute=False))[0].y
    assert np.array_equal(fresh, first) and np.load(path).shape == x.shape  # other shape: recomputed and stored again
    redo = algo.run(x, ["bfp4"], Quantizer("emulation"), _cache(tmp_path, recompute=True))[0].y
    assert np.array_equal(redo, first)


def test_wq_emulation_prints_transpose_rows(tmp_path):
    out = subprocess.run([sys.executable, str(ROOT / "wq"), "synthetic:gpt2", "h.0.attn.c_attn.weight", "--backend", "emulation",
                          "--compression-config", str(CONFIG), "--results-dir", str(tmp_path), "--no-plots"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert "compression: none, transpose" in lines
    rows = [ln.split() for ln in lines if ln.startswith("  none ") or ln.startswith("  transpose ")]
    assert [r[0] for r in rows] == ["none"] * 5 + ["transpose"] * 5
    assert [r[1] for r in rows] == [f.upper() for f in FORMATS] * 2
    assert rows[5][2:5] == rows[0][2:5]                                   # bf16 is elementwise: the same columns on both layouts
    assert rows[9][2:5] == rows[4][2:5]                                   # fp0 likewise


def test_capi_argument_checks_without_gpu():
    L = hb.lib()
    assert hasattr(L, "mtq_tile_stats_transposed") and hasattr(L, "mtq_quantize_transposed")
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ts, q = L.mtq_tile_stats_transposed, L.mtq_quantize_transposed
    assert ts(None, 0, 1, 0, 32, 32, 32, 0xF, p, None) == -1              # null x
    assert ts(p, 0, 1, 0, 32, 32, 32, 0xF, None, None) == -1              # null stats
    assert ts(p, 2, 1, 0, 32, 32, 32, 0xF, p, None) == -1                 # dtype
    assert ts(p, 0, 1, 0, 32, 32, 31, 0xF, p, None) == -1                 # ld < cols
    assert ts(p, 0, 0, 0, 32, 32, 32, 0xF, p, None) == -1                 # count < 1
    assert ts(p, 0, 1, 0, 32, 32, 32, 0x0, p, None) == -1                 # empty mask
    assert ts(p, 0, 1, 0, 0, 32, 32, 0xF, p, None) == -1                  # empty matrix
    assert q(None, 0, 32, 32, 32, 1, p, 32, None) == -1
    assert q(p, 0, 32, 32, 32, 1, None, 32, None) == -1
    assert q(p, 1, 32, 32, 31, 1, p, 32, None) == -1                      # ld < cols
    assert q(p, 1, 32, 32, 32, 1, p, 31, None) == -1                      # ldy < cols
    assert q(p, 5, 32, 32, 32, 1, p, 32, None) == -1                      # dtype
    assert q(p, 1, 32, 32, 32, 5, p, 32, None) == -4                      # unknown format: MTQ_ERR_UNSUPPORTED
    assert q(p, 1, 32, 32, 32, -1, p, 32, None) == -4
    assert b"format" in L.mtq_last_error()


def test_binding_rejects_bad_tensors():
    import torch

    x = torch.zeros((64, 48), dtype=torch.bfloat16)
    with pytest.raises(hb.MtqError, match="device tensor"):
        hb.tile_stats_transposed(x, 0xF)
    with pytest.raises(hb.MtqError, match="device tensor"):
        hb.quantize_transposed(x[:, ::2], "bfp8")


class _FakeCuda:
    """Stands in for a device tensor in the checks that come before any pointer is taken (rank, inner stride, storage type)."""

    def __init__(self, t):
        self.t, self.is_cuda = t, True
        self.dtype = t.dtype

    def dim(self):
        return self.t.dim()

    def stride(self, i):
        return self.t.stride(i)


def test_binding_checks_rank_stride_dtype():
    import torch

    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.quantize_transposed(_FakeCuda(torch.zeros((8, 8))[:, ::2]), "bfp8")
    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.tile_stats_transposed(_FakeCuda(torch.zeros((2, 8, 8))[:, :, ::2]), 0xF)
    with pytest.raises(hb.MtqError, match="2-D"):
        hb.quantize_transposed(_FakeCuda(torch.zeros((2, 8, 8))), "bfp8")
    with pytest.raises(hb.MtqError, match="2-D or 3-D"):
        hb.tile_stats_transposed(_FakeCuda(torch.zeros(8)), 0xF)
    with pytest.raises(hb.MtqError, match="bfloat16 or float32"):
        hb.tile_stats_transposed(_FakeCuda(torch.zeros((8, 8), dtype=torch.float16)), 0xF)


def test_binding_on_a_library_without_the_symbols(monkeypatch):
    """An older build of the same version (an A/B library at MTQ_LIB) lacks the transposed entry points: it still serves everything
    else, and a transposed call says to rebuild instead of failing with AttributeError."""
    real = hb.lib()

    class _OlderLibrary:
        def __getattr__(self, name):
            if name in hb.OPTIONAL_EXPORTS:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(hb, "lib", lambda: _OlderLibrary())
    assert hb.lib().mtq_version() == 143
    for name in hb.OPTIONAL_EXPORTS:
        with pytest.raises(hb.MtqError, match="rebuild"):
            hb._transposed_entry(name)
