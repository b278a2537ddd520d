"""The calibration kernels on the MI355X against the one right answer, bit for bit: mtq_gram_blocks, mtq_gram_full, mtq_tile_error_tables,
mtq_tile_error_tables_transposed and mtq_gptq_sweep on the exact-arithmetic cases of test_calibration_exact_host.py (which proves, in
integer arithmetic and without a GPU, that the float64 emulation of every case is exact and so independent of the summation order).

Every comparison is torch.equal or np.array_equal on the bits: no tolerance, no mask, every entry and every row.  What the rounding-bound
tests (test_budget_maps_gpu.py, test_gptq_gpu.py, test_output_error_transpose_gpu.py) cannot see shows here: one lost or doubled token
at a span, fold or step edge of the Gram kernels, a wrong tile on the second trip of the tables' grid-stride loops, and the sweep's rows
that sit on a tie, saturate, or take E from updated values.

References: the Gram kernels against a float64 matmul of the integer-valued X on the device (exact); the small table cases against the
host emulation, the large ones (grid-stride) against a float64 einsum on the device over K2's / K2T's own Δ (exact by the same bound,
tables_crude_bound); the sweep against gq.sweep_emulation and the host file's integer restatement."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from quantization_analysis_amd import budget_maps as bm
from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.layer_io import Chunk
from tests import test_calibration_exact_host as cx

pytestmark = pytest.mark.gpu
TILE = 32


# ----------------------------------------------------------------------------- Gram

def _gram_views(xi: torch.Tensor):
    """The same bf16 values behind two layouts: rows at an odd element offset (element-wise staging) and rows at a 16-byte-aligned offset
    with a row pitch that is a multiple of 8 elements (vector staging), both with ldx > k."""
    m, k = xi.shape
    x = cx.gram_tensor(xi)
    odd = torch.zeros((m, k + 8), dtype=torch.bfloat16, device=xi.device)
    odd[:, 1: 1 + k] = x
    al = torch.zeros((m, k + 16 + (-k) % 8), dtype=torch.bfloat16, device=xi.device)
    al[:, 8: 8 + k] = x
    odd, al = odd[:, 1: 1 + k], al[:, 8: 8 + k]
    assert odd.data_ptr() % 4 == 2 and al.data_ptr() % 16 == 0 and al.stride(0) % 8 == 0 and min(odd.stride(0), al.stride(0)) > k
    return odd, al


def _blocks_of(full: torch.Tensor, k: int) -> torch.Tensor:
    """The diagonal 32 × 32 blocks of a k × k matrix, zero padded: [ceil(k/32), 32, 32]."""
    nb = -(-k // TILE)
    p = torch.zeros((nb * TILE, nb * TILE), dtype=full.dtype, device=full.device)
    p[:k, :k] = full
    return torch.stack([p[b * TILE:(b + 1) * TILE, b * TILE:(b + 1) * TILE] for b in range(nb)])


def _block_ref(xd: torch.Tensor) -> torch.Tensor:
    m, k = xd.shape
    nb = -(-k // TILE)
    xp = torch.zeros((m, nb * TILE), dtype=torch.float64, device=xd.device)
    xp[:, :k] = xd
    xb = xp.view(m, nb, TILE).permute(1, 0, 2)
    return torch.bmm(xb.transpose(1, 2), xb)


def _gram_ms(kind: str, k: int) -> list:
    edges = cx.gram_edge_ms(kind, k)
    return sorted(set(cx.GRAM_M) | {m for _n, m, _s, _c in edges} | {cx.GRAM_M_LARGE})


@pytest.mark.parametrize("k", cx.GRAM_K)
def test_gram_kernels_equal_the_integer_gram(k):
    """Every m of the step, fold and span edges, both staging paths, added into a non-zero integer h; gram_full's diagonal blocks
    against gram_blocks' output."""
    torch.cuda.set_device(0)
    ms = {kind: _gram_ms(kind, k) for kind in ("blocks", "full")}
    big = cx.gram_ints(max(ms["blocks"] + ms["full"]), k, 1, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(k)
    h0_full = torch.randint(-1000, 1001, (k, k), generator=g, device="cuda").double()      # not symmetric: (a, b) and (b, a) are each added to
    h0_blocks = torch.randint(-1000, 1001, (-(-k // TILE), TILE, TILE), generator=g, device="cuda").double()
    for m in sorted(set(ms["blocks"]) | set(ms["full"])):
        xi = big[:m]
        xd = xi.double()
        want_full = xd.T @ xd
        want_blocks = _block_ref(xd)
        assert torch.equal(_blocks_of(want_full, k), want_blocks)
        for name, x in zip(("odd", "aligned"), _gram_views(xi)):
            if m in ms["full"]:
                h = hb.gram_full(x, h0_full.clone())
                assert torch.equal(h, h0_full + want_full), ("full", m, k, name, _first_diff(h, h0_full + want_full))
                hz = hb.gram_full(x, torch.zeros_like(h0_full))
                assert torch.equal(hz, hz.T)
            if m in ms["blocks"]:
                hbk = hb.gram_blocks(x, h0_blocks.clone())
                assert torch.equal(hbk, h0_blocks + want_blocks), ("blocks", m, k, name, _first_diff(hbk, h0_blocks + want_blocks))
            if m in ms["full"] and m in ms["blocks"]:
                assert torch.equal(_blocks_of(hz, k), hbk - h0_blocks)


def _first_diff(a, b):
    idx = torch.nonzero(a != b)
    return (int(idx.shape[0]), idx[0].tolist(), float(a[tuple(idx[0])]), float(b[tuple(idx[0])])) if idx.shape[0] else None


@pytest.mark.parametrize("k", cx.GRAM_K)
def test_gram_over_several_chunks(k):
    """gram_blocks_hip / gram_full_hip over uneven chunks, one of them empty, with the scratch carried from chunk to chunk."""
    torch.cuda.set_device(0)
    m = 2 * cx.GRAM_M_LARGE // 3 + 1
    xi = cx.gram_ints(m, k, 2, device="cuda")
    x = cx.gram_tensor(xi)
    cuts = [0, 1, 1, 257, 257 + 513, m - 64, m]
    chunks = [Chunk(x=x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    xd = xi.double()
    want = xd.T @ xd
    h, tokens = gq.gram_full_hip(chunks, k)
    assert tokens == m and torch.equal(h, want), _first_diff(h, want)
    hbk, tokens = bm.gram_blocks_hip(chunks, k)
    assert tokens == m and torch.equal(hbk, _blocks_of(want, k))


def test_gram_full_at_the_down_proj_width():
    """k = 18432 (h and the reference are 2.7 GB each): one span, 10440 super-block pairs, a few tokens."""
    torch.cuda.set_device(0)
    k = 18432
    assert cx.gram_spans("full", 65, k) == 1
    for m in (65, 257):
        xi = cx.gram_ints(m, k, 3, device="cuda")
        h = hb.gram_full(_gram_views(xi)[m % 2], torch.zeros((k, k), dtype=torch.float64, device="cuda"))
        xd = xi.double()
        want = xd.T @ xd
        assert torch.equal(h, want), (m, _first_diff(h, want))
        del h, want


# ----------------------------------------------------------------------------- tile error tables

def _tables(w, h, layout, want_weight=True):
    fn = hb.tile_error_tables_transposed if layout == "transpose" else hb.tile_error_tables
    return fn(w, h, want_weight=want_weight)


@pytest.mark.parametrize("layout", ["rows", "transpose"])
@pytest.mark.parametrize("hkind", ["gram", "dense"])
@pytest.mark.parametrize("n,k", cx.TABLE_SHAPES)
def test_tables_equal_the_exact_tables(n, k, hkind, layout):
    torch.cuda.set_device(0)
    h = cx.tables_h(k, hkind, 0)
    hd = torch.from_numpy(h).cuda()
    for wdt in ("bf16", "f32"):
        w = cx.tables_view(cx.tables_weight(n, k, 0), k, wdt, device="cuda")
        assert w.stride(0) > k and w.storage_offset() == 2
        want_out, want_w = bm.tile_error_tables_emulation(w.cpu(), h, layout)
        for wv in (w, w.contiguous()):
            e_out, e_w = _tables(wv, hd, layout)
            assert np.array_equal(e_out.cpu().numpy().view(np.uint64), want_out.view(np.uint64)), (wdt, np.nonzero(e_out.cpu().numpy() != want_out))
            assert np.array_equal(e_w.cpu().numpy().view(np.uint64), want_w.view(np.uint64)), wdt
            only, none = _tables(wv, hd, layout, want_weight=False)
            assert none is None and torch.equal(only, e_out)
        if hkind == "gram" and layout == "rows":                 # through the public route, from the kernel's own (exact) H
            got_out, got_w = bm.tile_error_tables_hip(w, hd, layout)
            assert np.array_equal(got_out, want_out) and np.array_equal(got_w, want_w)


def _tables_device_ref(w, hd, layout):
    """budget_maps' tables in float64 on the device from K2's (K2T's) Δ: exact where tables_crude_bound < 2⁵³."""
    n, k = w.shape
    th, tw = bm.tiles_hw(n, k)
    e_out = torch.zeros((th * tw, 4), dtype=torch.float64, device=w.device)
    e_w = torch.zeros_like(e_out)
    wc = w.contiguous()
    for code, f in enumerate(cx.ALL):
        q = hb.quantize_transposed(wc, f) if layout == "transpose" else hb.quantize(wc, f)
        d = torch.zeros((th * TILE, tw * TILE), dtype=torch.float64, device=w.device)
        d[:n, :k] = q.double() - wc.double()
        dt = d.view(th, TILE, tw, TILE).permute(2, 0, 1, 3).reshape(tw, th * TILE, TILE)    # [c, (r, i), a]
        g = torch.bmm(dt, hd)                                                             # (δ_iᵀ H_c)[b]
        so = (g * dt).reshape(tw, th, TILE * TILE).sum(dim=2)                                 # [c, r]
        sw = (dt * dt).reshape(tw, th, TILE * TILE).sum(dim=2)
        e_out[:, code] = (so if layout == "transpose" else so.T).reshape(-1)
        e_w[:, code] = (sw if layout == "transpose" else sw.T).reshape(-1)
    return e_out, e_w


def test_device_reference_equals_the_emulation():
    """The large cases' reference, checked on a small case against the host emulation (itself equal to the int64 tables)."""
    torch.cuda.set_device(0)
    n, k = 300, 200
    h = cx.tables_h(k, "dense", 0)
    w = cx.tables_view(cx.tables_weight(n, k, 0), k, "f32", device="cuda")
    for layout in ("rows", "transpose"):
        want_out, want_w = bm.tile_error_tables_emulation(w.cpu(), h, layout)
        ref_out, ref_w = _tables_device_ref(w, torch.from_numpy(h).cuda(), layout)
        assert np.array_equal(ref_out.cpu().numpy(), want_out) and np.array_equal(ref_w.cpu().numpy(), want_w)


@pytest.mark.parametrize("layout", ["rows", "transpose"])
@pytest.mark.parametrize("n,k,hkind,wdt", cx.TABLE_LARGE)
def test_tables_where_the_grid_stride_loop_iterates(n, k, hkind, wdt, layout):
    torch.cuda.set_device(0)
    th, tw = bm.tiles_hw(n, k)
    assert th > 16384 // tw
    hd = torch.from_numpy(cx.tables_h(k, hkind, 0)).cuda()
    w = cx.tables_view(cx.tables_weight(n, k, 0), k, wdt, device="cuda")
    want_out, want_w = _tables_device_ref(w, hd, layout)
    e_out, e_w = _tables(w, hd, layout)
    assert torch.equal(e_out, want_out), _first_diff(e_out, want_out)
    assert torch.equal(e_w, want_w), _first_diff(e_w, want_w)
    assert int((want_out != 0).any(dim=1).sum()) > 0.9 * th * tw


# ----------------------------------------------------------------------------- the sweep

def _sweep_both(w, u, codes):
    """The sweep on the device with U as given and with NaN below U's diagonal (only the upper triangle may be read) → Ŵ, loss."""
    what, loss = gq.sweep_hip(w, u, codes)
    k = u.shape[0]
    poisoned = np.where(np.tri(k, k, -1, dtype=bool), np.nan, u)
    what2, loss2 = gq.sweep_hip(w, poisoned, codes)
    got, got_loss = what.cpu().numpy(), loss.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), what2.cpu().numpy().view(np.uint32))
    assert np.array_equal(got_loss.view(np.uint64), loss2.cpu().numpy().view(np.uint64))
    return got, got_loss


def _check_sweep(w32, u, codes, k, wdt):
    w = cx.sweep_view(w32, k, wdt, device="cuda")
    assert w.shape[1] == k and (w32.shape[1] == k or (w.stride(0) > k and w.storage_offset() == 1))
    want, want_loss, _margin = gq.sweep_emulation(w.cpu(), u, codes)
    q, loss, ev = cx.sweep_int(w.float().cpu().numpy(), u, codes)
    assert np.array_equal(want.view(np.uint32), q.view(np.uint32)) and np.array_equal(want_loss.view(np.uint64), loss.view(np.uint64))
    got, got_loss = _sweep_both(w, u, codes)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) | (got_loss.view(np.uint64) != want_loss.view(np.uint64)))[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (bad, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
    assert np.array_equal(got_loss.view(np.uint64), want_loss.view(np.uint64)), bad
    cont, cont_loss = gq.sweep_hip(w.contiguous(), u, codes)
    assert np.array_equal(cont.cpu().numpy().view(np.uint32), got.view(np.uint32)) and np.array_equal(cont_loss.cpu().numpy(), got_loss)
    if not any(ev[c]["saturated"] for c in (1, 2, 3)):           # grid membership, where no element left its group's range
        assert np.array_equal(bm.reconstruct_emulation(got, codes).view(np.uint32), got.view(np.uint32))
    return ev


@pytest.mark.parametrize("n,k", cx.SWEEP_SHAPES)
def test_sweep_equals_the_exact_sweep_on_every_row(n, k):
    torch.cuda.set_device(0)
    for nn, kk, wdt, kind in cx.sweep_family():
        if (nn, kk) != (n, k):
            continue
        w32, u = cx.sweep_case(n, k, wdt)
        _check_sweep(w32, u, cx.sweep_codes(n, k, kind), k, wdt)
    for wdt in ("bf16", "f32"):                                  # both storages under the mixed map, contiguous rows with ldw == k
        w32, u = cx.sweep_case(n, k, wdt, pad=0)
        _check_sweep(w32, u, cx.sweep_codes(n, k, "map"), k, wdt)


@pytest.mark.parametrize("code", [1, 2, 3])
def test_sweep_saturates_as_the_contract_says(code):
    torch.cuda.set_device(0)
    w32, u, codes = cx.forced_case(code)
    for wdt in ("bf16", "f32"):
        ev = _check_sweep(w32, u, codes, cx.FORCED_K, wdt)
        assert ev[code]["saturated"] >= 16 and ev[code]["current_e"] >= 4


def test_sweep_long_rows():
    torch.cuda.set_device(0)
    n, k, kind = cx.SWEEP_LONG
    w32, u = cx.sweep_case(n, k, "bf16")
    _check_sweep(w32, u, cx.sweep_codes(n, k, kind), k, "bf16")
