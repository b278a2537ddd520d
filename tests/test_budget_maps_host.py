"""Budget maps on the host: the float64 emulation tables against a brute-force output error per tile, the allocation rule against every
assignment of small tables, the activation-aware map's quality, the CLI's budget rows and the new C entry points' argument checks."""
from __future__ import annotations

import itertools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_BYTES_PER_ELEM, MIXED_TILE_FORMATS, mixed_tile_total_bytes
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import emulation_sums
from quantization_analysis_amd.quantization_formats import quantize_weight_values
from tests.test_output_error_host import make_fixture

ROOT = Path(__file__).resolve().parent.parent
ALL = list(MIXED_TILE_FORMATS)


@pytest.mark.parametrize("n,k,wdt", [(64, 96, "f32"), (50, 70, "bf16"), (33, 40, "f32"), (5, 16, "bf16")])
def test_emulation_tables_match_brute_force(n, k, wdt):
    rng = np.random.default_rng(n * 100 + k)
    w = torch.from_numpy((rng.standard_normal((n, k)) * 0.05).astype(np.float32))
    w = w.to(torch.bfloat16) if wdt == "bf16" else w
    x = torch.from_numpy(rng.standard_normal((45, k)).astype(np.float32)).to(torch.bfloat16)
    h, m = bm.gram_blocks_emulation([Chunk(x=x[:20]), Chunk(x=x[20:])], k)
    assert m == 45 and h.shape == (-(-k // 32), 32, 32)
    e_out, e_w = bm.tile_error_tables_emulation(w, h)
    th, tw = bm.tiles_hw(n, k)
    x64 = x.double().numpy()
    w32 = w.float().numpy()
    for code, f in enumerate(ALL):
        d = quantize_weight_values(w32, f).astype(np.float64) - w32.astype(np.float64)
        for r in range(th):
            for c in range(tw):
                dt = d[32 * r: 32 * r + 32, 32 * c: 32 * c + 32]
                xc = x64[:, 32 * c: 32 * c + dt.shape[1]]
                want = float(((xc @ dt.T) ** 2).sum())           # ‖X_c·Δ_tᵀ‖²_F
                got = e_out[r * tw + c, code]
                assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (f, r, c, got, want)
                assert abs(e_w[r * tw + c, code] - float((dt ** 2).sum())) <= 1e-12 * float((dt ** 2).sum()) + 1e-300


def _brute_force(e, formats, bits):
    """Every assignment of the candidate formats → (bytes, Σe) of each."""
    T = e.shape[0]
    codes = [ALL.index(f) for f in ALL if f in formats]
    out = []
    for combo in itertools.product(codes, repeat=T):
        counts = {f: combo.count(i) for i, f in enumerate(ALL)}
        out.append((mixed_tile_total_bytes(counts), float(e[np.arange(T), list(combo)].sum())))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_allocation_is_optimal_for_its_bytes(seed):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 7))
    e = rng.random((T, 4)) * rng.choice([1.0, 10.0, 1000.0], size=(T, 4))
    if seed % 3 == 0:
        e = np.round(e)                                             # ties
    fmts = ALL if seed % 4 else ["bfp8", "bfp4", "bfp2"]
    prev = np.inf
    allc = _brute_force(e, fmts, 16)
    for bits in (1.5, 2.0, 3.0, 4.5, 6.0, 9.0, 12.0, 16.0):
        got = bm.allocate(e, fmts, bits, (1, T))
        if isinstance(got, str):
            assert "below" in got and bits < 8 * MIXED_TILE_BYTES_PER_ELEM[fmts[-1]] + 1
            continue
        a, counts, tb = got
        assert a.dtype == np.int8 and a.shape == (1, T) and set(np.unique(a)) <= {ALL.index(f) for f in fmts}
        assert tb <= bits / 8 * 1024 * T and tb == mixed_tile_total_bytes(counts)
        s = float(e[np.arange(T), a.reshape(-1).astype(int)].sum())
        best = min(v for b, v in allc if b <= tb)
        assert s <= best + 1e-12 * max(1.0, abs(best)), (bits, s, best)
        assert s <= prev + 1e-12 * max(1.0, abs(prev))              # Σe does not grow with the budget
        prev = s


def test_sixteen_bits_takes_each_tiles_least_error_cheapest_on_ties():
    e = np.array([[1.0, 1.0, 3.0, 4.0],      # bf16 ties bfp8 → bfp8
                  [5.0, 2.0, 2.0, 2.0],      # bfp8 / bfp4 / bfp2 tie → bfp2
                  [0.0, 1.0, 2.0, 3.0],      # bf16
                  [9.0, 3.0, 1.0, 2.0]])     # bfp4
    a, counts, tb = bm.allocate(e, ALL, 16, (2, 2))
    assert a.tolist() == [[1, 3], [0, 2]]
    assert counts == {"bf16": 1, "bfp8": 1, "bfp4": 1, "bfp2": 1}


def test_zero_tables_keep_the_cheapest_format():
    z = np.zeros((6, 4))
    for fmts, want in ((ALL, 3), (["bf16", "bfp8"], 1), (["bf16", "fp0"], 0)):
        a, counts, tb = bm.allocate(z, fmts, 16, (2, 3))
        assert (a == want).all() and counts[ALL[want]] == 6


def test_reasons():
    e = np.ones((4, 4))
    assert "no mixed-tile format" in bm.allocate(e, ["fp0"], 4)
    assert "below the all-bfp8 size" in bm.allocate(e, ["bf16", "bfp8"], 4)     # 8 · 1.088 > 4
    assert isinstance(bm.allocate(e, ["bf16", "bfp8"], 8.8), tuple)
    bad = e.copy()
    bad[2, 1] = np.nan
    assert "non-finite" in bm.allocate(bad, ALL, 4)
    bad[2, 1] = np.inf
    assert "non-finite" in bm.allocate(bad, ALL, 4)
    for b in (0, -1, 16.5):
        with pytest.raises(ValueError, match=r"\(0, 16\]"):
            bm.allocate(e, ALL, b)


def quality_case(seed: int, tokens: int = 4096):
    """W 256 × 256 ~ N(0, 0.02); X ~ N(0, 1) with two outlier channels ×30 in one 32-column block; calibration and evaluation
    tokens drawn separately."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(256, 256, generator=g) * 0.02

    def acts():
        x = torch.randn(tokens, 256, generator=g)
        x[:, 70] *= 30.0
        x[:, 77] *= 30.0
        return x.to(torch.bfloat16)

    return w, acts(), acts()


def loe_sse(sums) -> float:
    """Σ(r − q)² of the LOE sums of one slot: Σr² − 2Σrq + Σq²."""
    return float(sums[1] - 2.0 * sums[4] + sums[3])


def test_quality_output_map_beats_weight_map():
    w, x_cal, x_eval = quality_case(1)
    h, _ = bm.gram_blocks_emulation([Chunk(x=x_cal)], 256)
    e_out, e_w = bm.tile_error_tables_emulation(w, h)
    for bits in (3.0, 4.5, 6.0):
        sse = {}
        for basis, table in (("output", e_out), ("weight", e_w)):
            a, _counts, tb = bm.allocate(table, ALL, bits, (8, 8))
            assert tb <= bits / 8 * 1024 * 64
            sums, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, bm.reconstruct_emulation(w, a))
            sse[basis] = loe_sse(sums[4])
        assert sse["weight"] >= 2.0 * sse["output"], (bits, sse)


def _run(args, cwd=ROOT):
    return subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), *args], capture_output=True, text=True,
                          cwd=cwd, timeout=600)


def test_cli_budget_rows(tmp_path):
    model, io = make_fixture(tmp_path)
    base = [str(model), str(io), "model.layers.0", "--backend", "emulation", "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--split", "test"]
    r0 = _run(base + ["--out-dir", str(tmp_path / "plain")])
    r1 = _run(base + ["--out-dir", str(tmp_path / "budget"), "--budget-bits", "3", "4.5", "--save-maps"])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    d0 = json.loads((tmp_path / "plain" / "layer_output_error.json").read_text())
    d1 = json.loads((tmp_path / "budget" / "layer_output_error.json").read_text())
    assert "budget_bits" not in d0 and d1["budget_bits"] == [3.0, 4.5] and d1["calib_split"] == "calibration" and d1["calib_io"] == str(io)
    for o0, o1 in zip(d0["ops"], d1["ops"]):
        assert o0["op"] == o1["op"]
        assert o1["rows"][: len(o0["rows"])] == o0["rows"]                  # the rows without the flags, unchanged
        extra = o1["rows"][len(o0["rows"]):]
        assert [x["candidate"] for x in extra] == ["budget:3:output", "budget:3:weight", "budget:4.5:output", "budget:4.5:weight"]
        n, k = o1["shape"]
        T = -(-n // 32) * -(-k // 32)
        for x in extra:
            assert x["basis"] in ("output", "weight") and x["bits"] in (3.0, 4.5)
            assert x["bytes"] <= x["bits"] / 8 * 1024 * T and x["calib_tokens"] > 0 and x["predicted_sse_calib"] >= 0.0
            assert 0.0 < x["pcc"] <= 1.0
        assert o1["calib_splits"] == ["calibration"] and o1["budget_skipped"] == []
    csv0 = (tmp_path / "plain" / "layer_output_error.csv").read_text().splitlines()
    csv1 = (tmp_path / "budget" / "layer_output_error.csv").read_text().splitlines()
    assert csv1[0] == csv0[0] and len(csv1) == len(csv0) + 2 * 4
    # the saved maps rebuild Ŵ through the reconstruct script
    op = "model.layers.0.mlp.down_proj"
    npy = tmp_path / "budget" / "maps" / op / "budget_4.5_output.npy"
    a = np.load(npy)
    assert a.dtype == np.int8 and a.shape == (1, 3)
    out = tmp_path / "recon.npy"
    rr = subprocess.run([sys.executable, str(ROOT / "scripts" / "reconstruct_mixed_tile_assignment.py"), str(model), f"{op}.weight", str(npy),
                         "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert rr.returncode == 0, rr.stderr
    from safetensors.torch import load_file

    w = load_file(str(model / "m.safetensors"))[f"{op}.weight"]
    assert np.array_equal(np.load(out).view(np.uint32), bm.reconstruct_emulation(w, a).view(np.uint32))


def test_cli_budget_without_calibration_samples_and_argument_errors(tmp_path):
    model, io = make_fixture(tmp_path, n_cal=0, n_test=2)
    r = _run([str(model), str(io), "model.layers.0.mlp.up_proj", "--split", "test", "--budget-bits", "4", "--out-dir", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    doc = json.loads((tmp_path / "o" / "layer_output_error.json").read_text())
    up = doc["ops"][0]
    assert not any(x["candidate"].startswith("budget:") for x in up["rows"])
    assert [x["candidate"] for x in up["budget_skipped"]] == ["budget:4:output", "budget:4:weight"]
    assert "no calibration samples" in up["budget_skipped"][0]["reason"] and "budget:4:output" in r.stdout
    for bad in (["--budget-bits", "4", "--x-format", "bfp8"], ["--budget-bits", "0"], ["--budget-bits", "17"]):
        r = _run([str(model), str(io), "up_proj", *bad, "--out-dir", str(tmp_path / "e")])
        assert r.returncode == 2 and "--budget-bits" in r.stderr, (bad, r.stderr)


def test_c_entry_points_check_arguments():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    assert L.mtq_gram_blocks_scratch_doubles(0, 32) == 0
    sz = L.mtq_gram_blocks_scratch_doubles(1000, 40)
    assert sz >= 2 * 1024 and sz % (2 * 1024) == 0
    ok = (p, 1000, 40, 40, p, 2048, p, sz, None)

    def gram(**kw):
        args = dict(zip(("x", "m", "k", "ldx", "h", "hd", "s", "sd", "st"), ok))
        args.update(kw)
        return L.mtq_gram_blocks(*args.values())

    assert gram(x=None) == -1 and b"null" in L.mtq_last_error()
    assert gram(h=None) == -1 and gram(s=None) == -1
    assert gram(ldx=39) == -1 and b"ldx < k" in L.mtq_last_error()
    assert gram(hd=1024) == -1 and b"h_doubles" in L.mtq_last_error()
    assert gram(sd=sz - 1) == -1 and b"scratch" in L.mtq_last_error()
    assert gram(m=0) == -1
    okt = (p, 0, 50, 40, 40, p, 2048, p, p, 2 * 2 * 4, None)

    def tables(**kw):
        args = dict(zip(("w", "dt", "n", "k", "ldw", "h", "hd", "eo", "ew", "td", "st"), okt))
        args.update(kw)
        return L.mtq_tile_error_tables(*args.values())

    assert tables(w=None) == -1 and b"null" in L.mtq_last_error()
    assert tables(h=None) == -1 and tables(eo=None) == -1
    assert tables(dt=5) == -1 and b"w_dtype" in L.mtq_last_error()
    assert tables(ldw=39) == -1 and b"ldw < k" in L.mtq_last_error()
    assert tables(hd=3072) == -1 and b"h_doubles" in L.mtq_last_error()
    assert tables(td=15) == -1 and b"table_doubles" in L.mtq_last_error()
    assert tables(n=0) == -1


def test_python_wrappers_check_arguments():
    x = torch.zeros((4, 40), dtype=torch.bfloat16)
    h = torch.zeros((2, 32, 32), dtype=torch.float64)
    with pytest.raises(hb.MtqError):
        hb.gram_blocks(x, h)                                    # host tensors
    with pytest.raises(hb.MtqError):
        hb.gram_blocks(x.float(), h)
    with pytest.raises(hb.MtqError):
        hb.gram_blocks(x.t(), h)
    with pytest.raises(hb.MtqError):
        hb.tile_error_tables(torch.zeros((8, 40)), h)
    with pytest.raises(hb.MtqError):
        hb.tile_error_tables(torch.zeros((8, 40), dtype=torch.float16), h)
