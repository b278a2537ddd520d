"""CPU-only: the mxfp4 / nvfp4 proxies on the host (quantization_formats.py) against the reference's own y bits (F17,
tests/golden/make_golden_fp4_proxy.py), the float32-log2 rule they and csrc/mtq_fp4_proxy.hip share against NumPy's log2, `wq
--backend emulation` with the two new rows, and the argument checks of the new C entry points and their binding."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import cli
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import quantization_formats as qf
from quantization_analysis_amd.compression_algorithms.quantizer import Quantizer
from tests.inputs import gen, sha

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
PROXIES = ["mxfp4", "nvfp4"]


@pytest.fixture(scope="module")
def f17():
    return np.load(GOLDEN / "f17_fp4_proxy.npz")


@pytest.fixture(scope="module")
def meta17():
    return json.loads((GOLDEN / "golden_meta_f17.json").read_text())


def same_bits(y: np.ndarray, want_bits: np.ndarray) -> np.ndarray:
    """Element-wise: equal bits (so the sign of zero counts), or both NaN."""
    want = want_bits.view(np.float32)
    return (y.view(np.uint32) == want_bits) | (np.isnan(y) & np.isnan(want))


@pytest.mark.parametrize("fmt", PROXIES)
def test_emulation_equals_the_reference_bits(f17, fmt):
    x = f17["x"].view(np.float32)
    y = qf.quantize_weight_values(x, fmt)
    ok = same_bits(y, f17[fmt])
    assert ok.all(), (fmt, x[~ok][:8], y[~ok][:8], f17[fmt][~ok][:8].view(np.float32))
    # the quirks the issue lists are in the fixture and hold here too
    probe = np.float32([1535.99988, 1535.99976, 3.4e38, np.inf, -np.inf, np.nan, -0.0, 0.005, -1e-45])
    got = qf.quantize_weight_values(probe, fmt)
    if fmt == "nvfp4":
        assert got[0] == 1440.0 and got[1] == 768.0 and got[7] == 0.0
    else:
        assert np.isinf(got[2])
    assert np.isnan(got[3:6]).all()
    assert got[6] == 0.0 and not np.signbit(got[6]) and np.signbit(got[8]) and got[8] == 0.0


def test_log2_rule_matches_numpy_float32_log2():
    """floor / ceil of np.log2 in float32 on the first and last 64 mantissas of every binade (subnormals included) equal the rule
    derived from the exponent bits, and the rule differs from the bare exponent there (so it is not vacuous)."""
    m = np.concatenate([np.arange(64), np.arange((1 << 23) - 64, 1 << 23)]).astype(np.uint32)
    s = ((np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)) | m[None, :]).ravel().view(np.float32)
    s = s[s > 0]
    floor, ceil = qf._log2_floor_ceil(s)
    ref = np.log2(s)
    assert ref.dtype == np.float32
    assert np.array_equal(floor, np.floor(ref).astype(np.int64))
    assert np.array_equal(ceil, np.ceil(ref).astype(np.int64))
    bare = np.floor(np.log2(s.astype(np.float64))).astype(np.int64)
    assert (floor != bare).sum() > 1000 and (ceil != bare + (s != np.exp2(bare))).sum() > 1000


@pytest.mark.parametrize("fmt", PROXIES)
def test_quantizer_emulation_takes_the_proxies(fmt):
    x = gen("heavy_f32", 7, (33, 47))
    y = Quantizer("emulation").quantize(x, fmt)
    assert y.shape == x.shape and y.dtype == np.float32
    assert np.array_equal(y.view(np.uint32), qf.quantize_weight_values(x, fmt).view(np.uint32))
    assert fmt in qf.SUPPORTED_FORMATS and qf.ROW_FORMATS.index(fmt) == 5 + PROXIES.index(fmt)


def test_default_format_list_is_the_references():
    assert qf.SUPPORTED_FORMATS == ["mxfp4", "nvfp4", "bf16", "bfp8", "bfp4", "bfp2", "fp0"]
    assert qf.ROW_FORMATS[:5] == ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]   # the row codes of the earlier formats stay
    assert cli.FORMAT_BYTES_PER_ELEM["mxfp4"] == cli.FORMAT_BYTES_PER_ELEM["nvfp4"] == 0.5


def write_recipe_model(meta17, tmp_path: Path) -> tuple[Path, dict]:
    """The F17 recipe tensors as a local safetensors model (bf16 storage for the bf16-valued one) → (directory, name → recipe)."""
    from safetensors.torch import save_file

    tensors, recipes = {}, {}
    for i, r in enumerate(meta17["recipes"]):
        x = gen(r["kind"], r["seed"], tuple(r["shape"]))
        assert sha(x) == r["x_sha256"]
        t = torch.from_numpy(x)
        name = f"model.layers.{i}.proj.weight"
        tensors[name] = t.to(torch.bfloat16) if r["kind"].endswith("bf16") else t
        recipes[name] = r
    d = tmp_path / "model"
    d.mkdir()
    save_file(tensors, str(d / "model.safetensors"))
    return d, recipes


def table_rows(table: str) -> dict:
    """{(tensor, FORMAT): (pcc, mae, atol)} of the `none` rows of a wq table."""
    out, name = {}, None
    for ln in table.splitlines():
        if ln and not ln.startswith(" "):
            name = ln.strip()
        m = re.match(r"\s+none\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s", ln)
        if m and name:
            out[(name, m.group(1))] = tuple(float(v) for v in m.group(2, 3, 4))
    return out


def run_wq(model: Path, tmp_path: Path, tag: str, formats, backend: str = "emulation", extra=()) -> dict:
    cfg = {"algorithm": "none"}
    if formats is not None:
        cfg["quantization_formats"] = formats
    p = tmp_path / f"{tag}.json"
    p.write_text(json.dumps(cfg))
    assert cli.run([str(model), "--compression-config", str(p), "--backend", backend, "--results-dir", str(tmp_path / tag), "--no-plots",
                    *extra]) == 0
    tables = list((tmp_path / tag).rglob("table.txt"))
    assert len(tables) == 1
    return table_rows(tables[0].read_text())


def check_against_f17(rows: dict, recipes: dict, pcc_tol: float = 1e-5):
    for name, r in recipes.items():
        for fmt in PROXIES:
            pcc, mae, atol = rows[(name, fmt.upper())]
            want = r["formats"][fmt]
            # the table prints 5 decimals / 4 significant digits: the reference's columns rounded as the table rounds them
            assert abs(pcc - want["pcc64"]) <= pcc_tol, (name, fmt, pcc, want)
            assert abs(mae - want["mae64"]) <= 5e-4 * want["mae64"] and abs(atol - want["atol32"]) <= 5e-4 * want["atol32"], (name, fmt)


def test_wq_emulation_prints_the_proxy_rows(meta17, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    model, recipes = write_recipe_model(meta17, tmp_path)
    named = run_wq(model, tmp_path, "named", ["nvfp4", "mxfp4"])
    assert {fmt for (_n, fmt) in named} == {"MXFP4", "NVFP4"}
    check_against_f17(named, recipes)
    default = run_wq(model, tmp_path, "default", None)
    assert {fmt for (_n, fmt) in default} == {f.upper() for f in qf.SUPPORTED_FORMATS}
    check_against_f17(default, recipes)
    for k, v in named.items():
        assert default[k] == v


def test_layer_output_error_still_rejects_the_proxies():
    from quantization_analysis_amd import output_error

    assert output_error.SUPPORTED_FORMATS == ["bf16", "bfp8", "bfp4", "bfp2", "fp0"]
    with pytest.raises(ValueError, match=r"Unsupported format\(s\) \['mxfp4'\]"):
        output_error.evaluate_op(None, None, ["bf16", "mxfp4"])


def test_c_entry_points_reject_bad_arguments():
    L = hb.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    n = int(L.mtq_fp4_proxy_scratch_doubles(1, 32, 32))
    assert n >= 12 and int(L.mtq_fp4_proxy_scratch_doubles(3, 32, 32)) == 3 * n and L.mtq_fp4_proxy_scratch_doubles(0, 32, 32) == 0
    sums = L.mtq_fp4_proxy_sums
    assert sums(None, 0, 1, 1024, 32, 32, 32, 3, p, p, 64, None) == -1 and b"null" in L.mtq_last_error()
    assert sums(p, 0, 1, 1024, 32, 32, 32, 3, None, p, 64, None) == -1
    assert sums(p, 0, 1, 1024, 32, 32, 32, 3, p, None, 64, None) == -1
    assert sums(p, 0, 1, 1024, 32, 32, 16, 3, p, p, 64, None) == -1 and b"ld < cols" in L.mtq_last_error()
    assert sums(p, 7, 1, 1024, 32, 32, 32, 3, p, p, 64, None) == -1 and b"in_dtype" in L.mtq_last_error()
    for mask in (0, 4, 7, 0x10):
        assert sums(p, 0, 1, 1024, 32, 32, 32, mask, p, p, 64, None) == -1 and b"fmt_mask" in L.mtq_last_error()
    assert sums(p, 0, 1, 1024, 0, 32, 32, 3, p, p, 64, None) == -1
    assert sums(p, 0, 2, 16, 32, 32, 32, 3, p, p, 64, None) == -1 and b"stride" in L.mtq_last_error()
    assert sums(p, 0, 1, 1024, 32, 32, 32, 3, p, p, n - 1, None) == -1 and b"scratch" in L.mtq_last_error()
    # mtq_quantize: the proxy codes check their arguments like the others; unknown codes stay unsupported
    assert L.mtq_quantize(None, 0, 32, 32, 32, 5, p, 32, None) == -1
    assert L.mtq_quantize(p, 0, 32, 32, 16, 6, p, 32, None) == -1
    assert L.mtq_quantize(p, 0, 32, 32, 32, 6, None, 32, None) == -1
    assert L.mtq_quantize(p, 9, 32, 32, 32, 5, p, 32, None) == -1
    assert L.mtq_quantize(p, 0, 32, 32, 32, 9, p, 32, None) == -4 and L.mtq_quantize(p, 0, 32, 32, 32, 7, p, 32, None) == -4
    # the transposed and map entry points keep refusing them
    assert L.mtq_quantize_transposed(p, 0, 32, 32, 32, 5, p, 32, None) == -4


class _FakeCuda:
    """Passes for a device tensor in the checks that come before any pointer is taken."""

    def __init__(self, t):
        self.t, self.is_cuda, self.dtype, self.shape = t, True, t.dtype, t.shape

    def dim(self):
        return self.t.dim()

    def stride(self, i):
        return self.t.stride(i)


def test_binding_checks_before_any_pointer():
    with pytest.raises(hb.MtqError, match="contiguous rows"):
        hb.fp4_proxy_sums(_FakeCuda(torch.zeros((8, 8))[:, ::2]), PROXIES)
    with pytest.raises(hb.MtqError, match="2-D or 3-D"):
        hb.fp4_proxy_sums(_FakeCuda(torch.zeros(8)), PROXIES)
    with pytest.raises(hb.MtqError, match="bfloat16 or float32"):
        hb.fp4_proxy_sums(_FakeCuda(torch.zeros((8, 8), dtype=torch.float16)), PROXIES)
    with pytest.raises(hb.MtqError, match="device tensor"):
        hb.fp4_proxy_sums(torch.zeros((8, 8)), PROXIES)   # a host tensor
    with pytest.raises(hb.MtqError, match="subset"):
        hb.fp4_proxy_sums(_FakeCuda(torch.zeros((8, 8))), ["bfp8"])
    with pytest.raises(ValueError, match="Unsupported"):
        hb.quantize_transposed(_FakeCuda(torch.zeros((8, 8))), "mxfp4")


class _HostAsDevice:
    """A host tensor that passes for a device tensor, with its real host pointer: a fake entry point can read it."""

    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


def test_sums_split_a_batch_into_launches_of_65535(monkeypatch):
    """More matrices than one launch takes: hb.fp4_proxy_sums hands the C entry point consecutive chunks of at most PROXY_MAX_COUNT
    matrices, each at its own x and out offset, with one chunk's scratch.  The fake entry point refuses what the C one refuses and
    writes Σx of every matrix it is given, read from the pointer it got, so a wrong offset shows as a wrong sum."""
    import ctypes

    count, rows, cols, ld = 2 * hb.PROXY_MAX_COUNT + 7, 2, 3, 5
    x = torch.arange(count * rows * ld, dtype=torch.float32).reshape(count, rows, ld) % 251
    view = x[:, :, :cols]                               # stride_elems = rows * ld, ld > cols
    per_matrix = 12 * 4                                 # any positive scratch size per matrix
    calls = []

    def scratch_doubles(n, r, c):
        assert (r, c) == (rows, cols)
        return n * per_matrix

    def sums(xp, code, n, stride, r, c, l, mask, outp, scratchp, scratch_n, stream):
        assert 0 < n <= hb.PROXY_MAX_COUNT and scratch_n >= n * per_matrix, "the C entry point refuses this"
        assert (code, stride, r, c, l, mask) == (hb.DTYPE_F32, rows * ld, rows, cols, ld, 3)
        calls.append((xp, n, outp, scratchp))
        xs = np.ctypeslib.as_array((ctypes.c_float * ((n - 1) * stride + (r - 1) * l + c)).from_address(xp))
        xs = np.concatenate([xs, np.zeros(n * stride - xs.size, np.float32)]).reshape(n, r, l)[:, :, :c]
        o = np.ctypeslib.as_array((ctypes.c_double * (n * 14)).from_address(outp)).reshape(n, 2, 7)
        o[:, :, 0] = xs.astype(np.float64).sum(axis=(1, 2))[:, None]
        return 0

    fakes = {"mtq_fp4_proxy_sums": sums, "mtq_fp4_proxy_scratch_doubles": scratch_doubles}
    monkeypatch.setattr(hb, "_entry", lambda name: fakes[name])
    monkeypatch.setattr(hb, "require_gpu", lambda: None)
    monkeypatch.setattr(hb, "_stream_ptr", lambda: 0)
    got = hb.fp4_proxy_sums(_HostAsDevice(view), PROXIES)
    M = hb.PROXY_MAX_COUNT
    offsets = [((xp - x.data_ptr()) // 4, n, (outp - got.data_ptr()) // 8) for xp, n, outp, _s in calls]
    assert offsets == [(0, M, 0), (M * rows * ld, M, M * 14), (2 * M * rows * ld, 7, 2 * M * 14)]
    assert len({c[3] for c in calls}) == 1
    want = view.double().sum(dim=(1, 2))
    assert torch.equal(got[:, 0, 0], want) and torch.equal(got[:, 1, 0], want)
    # a batch that fits takes one launch, and a 2-D tensor is a batch of one
    calls.clear()
    hb.fp4_proxy_sums(_HostAsDevice(view[:M]), PROXIES)
    hb.fp4_proxy_sums(_HostAsDevice(view[5]), PROXIES)
    assert [c[1] for c in calls] == [M, 1]
