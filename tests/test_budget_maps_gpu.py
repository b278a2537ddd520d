"""Budget maps on the MI355X: the Gram kernel against float64 within its contract's bound, the tile error tables against float64 from
the kernel's own H, hip maps against emulation maps where the cut has a slope margin above the tables' error, the budget rows' LOE,
the activation-aware map's quality and the CLI.  The exact cases (integer X and H, dyadic W: bit equality, every span, fold and step
edge of the Gram kernel, shapes where the tables' grid-stride loop iterates) are in test_calibration_exact_gpu.py."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.compression_algorithms.tile_utils import MIXED_TILE_FORMATS
from quantization_analysis_amd.layer_io import Chunk
from quantization_analysis_amd.output_error import SLOTS, emulation_sums, hip_sums
from tests.test_budget_maps_host import loe_sse, quality_case
from tests.test_output_error_gpu import _check, _eps
from tests.test_output_error_host import make_fixture

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ALL = list(MIXED_TILE_FORMATS)


def _gram64(x):
    """float64 H and |X|ᵀ|X| blocks of a device bf16 (m, k) tensor, on the device."""
    m, k = x.shape
    nb = -(-k // 32)
    xp = torch.zeros((m, nb * 32), dtype=torch.float64, device=x.device)
    xp[:, :k] = x.double()
    xb = xp.view(m, nb, 32).permute(1, 0, 2)                     # [nb, m, 32]
    return torch.bmm(xb.transpose(1, 2), xb), torch.bmm(xb.abs().transpose(1, 2), xb.abs())


@pytest.mark.parametrize("k", [32, 40, 7168])
@pytest.mark.parametrize("m,parts", [(1, 1), (17, 1), (1000, 1), (40000, 3)])
def test_gram_blocks_within_bound_and_deterministic(k, m, parts):
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(m * 31 + k)
    off = 1 if m % 2 else 0                                     # odd offset: the element-wise staging path; else ldx = k + 8, aligned
    base = (torch.randn((m, k + 8), generator=g, device="cuda") * 3).to(torch.bfloat16)
    x = base[:, off: off + k]
    assert x.stride(0) == k + 8 > k
    cuts = np.linspace(0, m, parts + 1).astype(int)
    h = torch.zeros((-(-k // 32), 32, 32), dtype=torch.float64, device="cuda")
    h2 = torch.zeros_like(h)
    for a, b in zip(cuts[:-1], cuts[1:]):
        hb.gram_blocks(x[a:b], h)
        hb.gram_blocks(x[a:b], h2)
    want, absx = _gram64(x)
    torch.cuda.synchronize()
    assert torch.equal(h, h2)
    err = (h - want).abs()
    assert bool((err <= 2.0 ** -15 * absx).all()), float((err / absx.clamp_min(1e-300)).max())


def _abs_quad(w32, h_abs):
    """Σ_i |δ_i|ᵀ h_abs_c |δ_i| per tile and format: the scale of the float64 error of e_out (h_abs = |H|, or |X|ᵀ|X|)."""
    from quantization_analysis_amd.quantization_formats import quantize_weight_values

    n, k = w32.shape
    th, tw = bm.tiles_hw(n, k)
    out = np.zeros((th * tw, 4))
    for code, f in enumerate(ALL):
        d = np.zeros((th * 32, tw * 32))
        d[:n, :k] = np.abs(quantize_weight_values(w32, f).astype(np.float64) - w32.astype(np.float64))
        dt = d.reshape(th, 32, tw, 32)
        out[:, code] = np.einsum("ricb,ricb->rc", np.einsum("rica,cab->ricb", dt, h_abs), dt).reshape(-1)
    return out


@pytest.mark.parametrize("n,k,wdt", [(70, 100, "f32"), (64, 96, "bf16"), (33, 7, "f32"), (300, 200, "bf16")])
def test_tile_error_tables_match_float64(n, k, wdt):
    torch.cuda.set_device(0)
    rng = np.random.default_rng(n + k)
    w = (rng.standard_normal((n, k + 5)) * 0.05).astype(np.float32)
    w[3, :16] = 0.0                                              # an all-zero group
    w[5, 16:32] *= 2.0 ** -110                                   # exponents outside the fast window, both ends
    w[6, :16] *= 2.0 ** 70
    w[7, 32: 48] = 2.0 ** -130                                   # denormals
    wt = torch.from_numpy(w).to(torch.bfloat16 if wdt == "bf16" else torch.float32).cuda()[:, 2: 2 + k]   # ldw > k
    x = (torch.randn((300, k), device="cuda") * 2).to(torch.bfloat16)
    h, m = bm.gram_blocks_hip([Chunk(x=x)], k)
    e_out, e_w = bm.tile_error_tables_hip(wt, h)
    e_out2, _ = bm.tile_error_tables_hip(wt.contiguous(), h)
    assert np.array_equal(e_out.view(np.uint64), e_out2.view(np.uint64))
    hh = h.cpu().numpy()
    want_out, want_w = bm.tile_error_tables_emulation(wt.cpu(), hh)
    bound = _abs_quad(wt.float().cpu().numpy(), np.abs(hh))
    assert np.all(np.abs(e_out - want_out) <= 1e-12 * bound + 1e-300)
    assert np.all(np.abs(e_w - want_w) <= 1e-12 * want_w + 1e-300)
    assert np.isfinite(e_out).all()


def _table_error(w, x_list, k):
    """Bound of |e_out(hip) − e_out(float64 H)|: the Gram kernel's 2⁻¹⁶·|X|ᵀ|X| through the quadratic form (×2 for slack), plus the
    tables' own float64 error."""
    _, absx = _gram64(torch.cat([x.cuda() for x in x_list]))
    q = _abs_quad(w.float().cpu().numpy(), absx.cpu().numpy())
    return 2.0 ** -15 * q + 1e-12 * q


def _cut_margin(e, err, formats, assignment):
    """Slope of the last taken segment minus that of the first one not taken, and the error bound of that difference."""
    order, tiles, frm, to, slope = bm.hull_segments(e, [f for f in ALL if f in formats])
    pos = {ALL.index(f): i for i, f in enumerate(order)}
    a = np.array([pos[int(c)] for c in assignment.reshape(-1)])
    taken = to <= a[tiles]
    take = int(taken.sum())
    assert taken[:take].all() and not taken[take:].any()        # the taken segments are a prefix
    if take == 0 or take == tiles.size:
        return np.inf, 0.0
    db = lambda i: abs(1024 * (bm.MIXED_TILE_BYTES_PER_ELEM[order[to[i]]] - bm.MIXED_TILE_BYTES_PER_ELEM[order[frm[i]]]))
    codes = [ALL.index(f) for f in order]
    eb = lambda i: (err[tiles[i], codes[frm[i]]] + err[tiles[i], codes[to[i]]]) / db(i)
    return slope[take - 1] - slope[take], eb(take - 1) + eb(take)


def _maps_agree(w, x_cal, formats, bits_list):
    k = int(w.shape[1])
    th, tw = bm.tiles_hw(int(w.shape[0]), k)
    h_d, _ = bm.gram_blocks_hip([Chunk(x=x) for x in x_cal], k)
    e_hip, ew_hip = bm.tile_error_tables_hip(w.cuda(), h_d)
    h_e, _ = bm.gram_blocks_emulation([Chunk(x=x) for x in x_cal], k)
    e_emu, ew_emu = bm.tile_error_tables_emulation(w, h_e)
    err = _table_error(w, x_cal, k)
    assert np.all(np.abs(e_hip - e_emu) <= err)
    assert np.all(np.abs(ew_hip - ew_emu) <= 1e-12 * ew_emu + 1e-300)
    checked = 0
    for bits in bits_list:
        for basis, t_hip, t_emu, t_err in (("output", e_hip, e_emu, err), ("weight", ew_hip, ew_emu, 1e-12 * ew_emu + 1e-300)):
            gh, ge = bm.allocate(t_hip, formats, bits, (th, tw)), bm.allocate(t_emu, formats, bits, (th, tw))
            if isinstance(ge, str):
                assert gh == ge
                continue
            margin, bound = _cut_margin(t_emu, t_err, formats, ge[0])
            assert margin > bound, (bits, basis, margin, bound)
            assert np.array_equal(gh[0], ge[0]) and gh[2] == ge[2], (bits, basis)
            checked += 1
    return checked


def test_hip_maps_equal_emulation_maps_on_the_fixture(tmp_path):
    torch.cuda.set_device(0)
    from quantization_analysis_amd.layer_io import chunks, select_ops
    from quantization_analysis_amd.model_source import build_model_index

    model, io = make_fixture(tmp_path)
    index = build_model_index(str(model))
    ops, _ = select_ops(index, io, "model.layers.0.mlp", "calibration")
    for op in ops:
        w = index.load(op.weight)
        n, k = w.shape
        xs = [c.x for c in chunks(op, k, n)]
        assert _maps_agree(w, xs, ALL, (3.0, 5.0)) > 0


def test_quality_on_hip_and_maps_equal_emulation():
    torch.cuda.set_device(0)
    w, x_cal, x_eval = quality_case(1)
    assert _maps_agree(w, [x_cal], ALL, (3.0, 4.5, 6.0)) == 6
    h, _ = bm.gram_blocks_hip([Chunk(x=x_cal)], 256)
    e_out, e_w = bm.tile_error_tables_hip(w.cuda(), h)
    for bits in (3.0, 4.5, 6.0):
        sse = {}
        for basis, table in (("output", e_out), ("weight", e_w)):
            a, _counts, tb = bm.allocate(table, ALL, bits, (8, 8))
            assert tb <= bits / 8 * 1024 * 64
            got, *_ = hip_sums([Chunk(x=x_eval)], w, [], None, a)
            sse[basis] = loe_sse(got[SLOTS.index("map")])
            # the budget row's LOE: hip against emulation within the bounds of the LOE kernel's f32 accumulation
            y = bm.reconstruct_emulation(w, a)
            want, *_ = emulation_sums([Chunk(x=x_eval)], w, [], None, y)
            xf = x_eval.float().numpy()
            _check(got[SLOTS.index("map")], want[SLOTS.index("map")], float(4096 * 256), _eps(xf, [w.numpy()], None, 256),
                   _eps(xf, [y], None, 256), f"{bits}:{basis}")
        assert sse["weight"] >= 2.0 * sse["output"], (bits, sse)


def test_cli_hip_agrees_with_emulation(tmp_path):
    model, io = make_fixture(tmp_path)
    docs = {}
    for backend in ("emulation", "hip"):
        out = tmp_path / backend
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "layer_output_error.py"), str(model), str(io), "model.layers.0.mlp",
                            "--backend", backend, "-c", "bf16", "bfp8", "bfp4", "bfp2", "fp0", "--split", "test", "--budget-bits", "3", "5",
                            "--save-maps", "--out-dir", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        docs[backend] = json.loads((out / "layer_output_error.json").read_text())
    for oe, oh in zip(docs["emulation"]["ops"], docs["hip"]["ops"]):
        assert oe["op"] == oh["op"] and oe["M"] == oh["M"] and len(oe["rows"]) == len(oh["rows"])
        for re_, rh in zip(oe["rows"], oh["rows"]):
            assert re_["candidate"] == rh["candidate"] and re_["bytes"] == rh["bytes"]
            assert abs(re_["pcc"] - rh["pcc"]) < 1e-5, (oe["op"], re_, rh)
            for key in ("mae", "atol"):
                assert abs(re_[key] - rh[key]) <= 1e-5 * max(1.0, abs(re_[key])), (oe["op"], re_, rh)
            if "predicted_sse_calib" in re_:
                assert rh["calib_tokens"] == re_["calib_tokens"]
                assert abs(rh["predicted_sse_calib"] - re_["predicted_sse_calib"]) <= 1e-4 * re_["predicted_sse_calib"] + 1e-12
        for f in (tmp_path / "emulation" / "maps" / oe["op"]).glob("*.npy"):
            assert np.array_equal(np.load(f), np.load(tmp_path / "hip" / "maps" / oe["op"] / f.name))
