"""GPU: the grouped skinny GLU and the MoE decode entries with a wave per 32-row chunk (include/mtq_glu_chunked.h), and the modules on
them.  Bit equality throughout; the oracle is never the new code: the walking entries (hb.packed_glu_skinny_grouped and its matmul
twin, the walking *_gather and *_combine entries), moe_dispatch + the walking GLU, two packed.linear(kernel="skinny") calls and
glu_combine, and the default modules.

  glu      count = 5 experts of n = 72, k = 300 in both orientations, a random map per expert, separate gate and up arenas.  The four
           routings of tests/glu_chunked_cases.py (ordinary groups; a hot group of 130 rows with 9 chunks in 11 slots; the slot bound met
           exactly; a single row) in ONE test each, so that every test meets a group behind another group's chunks; splits 1, 2, 0 and
           tiles_w + 3, both output types, silu and none, with and without biases, X contiguous, pitched and from an odd element, Y
           pitched in sentinels, twice over a 0xFF workspace with sentinels behind it.  The hot routing chunk by chunk against the dense
           skinny pair at the effective split, and with gate and up exchanged (the bits change).  k = 2100 with a 35-row group (a second
           64-tile hand-out); n = 300 (the chunked reduce's second 256-column chunk); count = 300 with groups of 0, 1 and 40 rows (the plan's run of two, the search's bisection).
  guards   an arena cut short, a group's stream cut short by its own bases, map codes 4 and -1, group_rows that decrease, end past T
           or start below 0: the walking entry's bits on the same operands, sentinels whole; three overlapping all-T groups: sentinels
           and the rows of no group only.
  gather   against moe_dispatch + the walking GLU and against the walking *_gather entry: k = 128, 40, 300, topk 1, 2, 3, 8, a group
           with a second chunk, two empty experts, dropped ids, three views of x, a hand-made src.
  combine  against the walking *_combine entry: n = 8, 72, 200, 300, topk 1, 2, 3, 5, 8, 9, split 0 .. 3, expert_dtype x out_dtype, the
           three kinds of base, a -0.0 base over zero rows, a NaN workspace, a hand-made row_of, y at an aligned and an odd pitch.
  layer    128 -> 96 -> 64, both `stored`, both decode routes: decode_grouped_kernel="chunks" is the default module to the bit; a
           forward under torch's sync-debug mode "error".  PackedExpertsMLP(decode_grouped_kernel="chunks") on one kept workspace."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests import glu_chunked_cases as cases
from tests.inputs import gen
from tests.moe_cases import I32_MAX, I32_MIN, SENTINEL, _bf16_valued, _bf16_words, _want_plan
from tests.moe_fused_cases import COUNT, HIDDEN, K_IN, K_OUT, STORED, _weights, down_split, glu_split, layer_experts, pack_experts, x_vec
from tests.test_packed_moe_fused_gpu import (GATHER_ROUTINGS, _bf16_words_any, _bits, _combine_inputs, _layer_inputs, _routing, _sentinels,
                                             _x_views)

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
N, K = 72, 300                                            # 3 x 10 tiles, both ragged
TAIL = 256


@functools.lru_cache(maxsize=None)
def _experts(count, n, k, seed, stored):
    """`count` experts in one orientation → (the list of packed experts, hip_backend's (arena, maps, offsets, bases))."""
    pts = pack_experts(_weights(count, n, k, seed), seed + 3, stored, backend="hip")
    batch = packed.batch_to_device(packed.as_batch(pts))
    return pts, (batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev)


def _x(T, k, seed):
    return torch.from_numpy(_bf16_words(gen("normal_f32", seed, (T, k)) * 50)).cuda().view(BF16)


def _rows(rows):
    return torch.tensor(list(rows), dtype=torch.int32, device="cuda")


def _workspace(need, fill=0xFF):
    buf = torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[:need] = fill
    return buf[:need], buf


def _whole(buf):
    return bool((buf[-TAIL:] == SENTINEL).all())


def _walk(kn):
    return hb.packed_glu_matmul_skinny_grouped if kn else hb.packed_glu_skinny_grouped


def _chunked(kn):
    return functools.partial(hb.glu_grouped_chunked, kn=kn)


def _size(kn):
    return functools.partial(hb.glu_grouped_chunked_workspace_bytes, kn=kn)


def _covered(rows, T):
    r0, r1 = cases.clamp(rows, T)
    covered = np.zeros(T, dtype=bool)
    for a, b in zip(r0, r1):
        covered[a:b] = True
    return covered


def _x_view(x, kind):
    """x's words contiguous (0), as a 16-byte-row view of a wider buffer (1), from an odd element of a buffer (2)."""
    T, k = x.shape
    if kind == 0:
        return x
    ld, lead = (((k + 15) // 8 * 8, 0), (k + 3, 1))[kind - 1]
    buf = torch.full((lead + (T + 2) * ld,), float("nan"), dtype=BF16, device="cuda")
    view = buf[lead: lead + T * ld].view(T, ld)[:, :k]
    view.copy_(x)
    return view


def _compare(kn, x, rows, gate, up, count, n, k, act, bg, bu, dtype, split, xkind=0, twice=True, check_rows=True):
    """One walking call and the chunked call (twice over a 0xFF workspace) into pitched sentinels; → the chunked (T, n) view."""
    T = x.shape[0]
    r = _rows(rows)
    want = _sentinels(T + 2, n + 5, dtype)
    _walk(kn)(x, r, gate, up, count, n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype, out=want[:T, :n], split=split)
    need = _size(kn)(T, count, n, k, split)
    assert need == cases.plan_bytes(count) + hb.packed_glu_skinny_grouped_workspace_bytes(T, count, n, k, split)
    got = None
    for _ in range(2 if twice else 1):
        got = _sentinels(T + 2, n + 5, dtype)
        ws, buf = _workspace(need)
        y = _chunked(kn)(_x_view(x, xkind), r, gate, up, count, n, act=act, bias_gate=bg, bias_up=bu, out_dtype=dtype, out=got[:T, :n], split=split,
                         workspace=ws)
        assert y.data_ptr() == got.data_ptr()
        what = (kn, tuple(rows)[:8], act, bg is not None, str(dtype), split, xkind)
        assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:4])      # sentinels included
        assert _whole(buf), (what, "bytes behind the workspace were written")
    if check_rows:
        pad = got.view(torch.uint8).view(T + 2, -1)[:T]
        assert bool((pad[torch.from_numpy(~_covered(rows, T)).cuda()] == SENTINEL).all()), "a row of no group was written"
    return got[:T, :n]


# ----------------------------------------------------------------------------- the bit contract

def test_the_routings_take_the_paths_they_are_there_for():
    for rows in cases.ROUTINGS:
        T, count = rows[-1], len(rows) - 1
        cstart = cases.chunks(rows, T)
        assert cstart[-1] <= cases.slots(T, count) and len(cases.chunk_rows(rows, T)) == cstart[-1]
    assert (cases.chunks(cases.HOT, 200)[-1], cases.slots(200, 5)) == (9, 11)               # surplus slots: two waves a tile row return early
    assert cases.chunks(cases.EXACT, 99)[-1] == cases.slots(99, 3) == 6                      # the bound met exactly
    assert (cases.chunks(cases.ORDINARY, 70)[-1], cases.slots(70, 5)) == (5, 7) and cases.chunks(cases.SINGLE, 1)[-1] == 1
    for rows in (cases.ORDINARY, cases.HOT, cases.EXACT):                                      # a group with rows behind other groups' chunks
        cstart, sizes = cases.chunks(rows, rows[-1]), np.diff(rows)
        assert any(cstart[e] > 0 and sizes[e] > 0 for e in range(len(sizes)))
        assert max(sizes) > cases.CHUNK                                                        # a second chunk
    tiles = -(-K // 32)
    assert tiles == 10 and glu_split(200, 5, N, K, tiles + 3) == tiles and glu_split(200, 5, N, K, 2) == 2      # an effective split above 1


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("out_dtype", (F32, BF16))
def test_the_chunked_glu_is_the_walking_glu_bit_for_bit(out_dtype, stored):
    kn = stored == "transpose"
    tiles_w = -(-K // 32)
    for ri, rows in enumerate(cases.ROUTINGS):
        T, count = rows[-1], len(rows) - 1
        (_g, gate), (_u, up) = _experts(count, N, K, 30, stored), _experts(count, N, K, 40, stored)
        x = _x(T, K, 100 + ri)
        bias = [torch.from_numpy(gen("normal_f32", 60 + i, (count, N)) * 20).cuda() for i in range(2)]
        for si, split in enumerate((1, 2, 0, tiles_w + 3)):
            eff = glu_split(T, count, N, K, split)
            assert eff == (min(split, tiles_w) if split else eff)
            for act in ("silu", "none"):
                for bg, bu in ((None, None), (bias[0], bias[1])):
                    _compare(kn, x, rows, gate, up, count, N, K, act, bg, bu, out_dtype, split, xkind=(si + (bg is not None)) % 3)


@pytest.mark.parametrize("stored", STORED)
def test_the_hot_routing_chunk_by_chunk_is_the_dense_skinny_pair_and_gate_and_up_matter(stored):
    kn = stored == "transpose"
    rows, T, count = cases.HOT, 200, 5
    (gates, gate), (ups, up) = _experts(count, N, K, 30, stored), _experts(count, N, K, 40, stored)
    dense = packed.matmul if kn else packed.linear
    x = _x(T, K, 7)
    bias = [torch.from_numpy(gen("normal_f32", 60 + i, (count, N)) * 20).cuda() for i in range(2)]
    for split in (1, 0, 3):
        eff = glu_split(T, count, N, K, split)
        assert split == 0 or eff == split
        for dtype, name in ((F32, "float32"), (BF16, "bfloat16")):
            for bg, bu in ((None, None), (bias[0], bias[1])):
                ws, buf = _workspace(_size(kn)(T, count, N, K, split))
                y = _chunked(kn)(x, _rows(rows), gate, up, count, N, bias_gate=bg, bias_up=bu, out_dtype=dtype, split=split, workspace=ws)
                assert _whole(buf) and not bool(y[torch.from_numpy(~_covered(rows, T)).cuda()].any())
                for e, r0, m in cases.chunk_rows(rows, T):
                    g = dense(x[r0:r0 + m], gates[e], bias=None if bg is None else bg[e], out_dtype="float32", kernel="skinny", split=eff)
                    u = dense(x[r0:r0 + m], ups[e], bias=None if bu is None else bu[e], out_dtype="float32", kernel="skinny", split=eff)
                    want = hb.glu_combine(g, u, act="silu", out_dtype=dtype)
                    assert np.array_equal(_bits(y[r0:r0 + m]), _bits(want)), (split, eff, name, bg is not None, e, r0)
                swapped = _chunked(kn)(x, _rows(rows), up, gate, count, N, bias_gate=bg, bias_up=bu, out_dtype=dtype, split=split)
                assert not np.array_equal(_bits(swapped), _bits(y)), "gate and up exchanged gave the same bits"
                want = _walk(kn)(x, _rows(rows), up, gate, count, N, bias_gate=bg, bias_up=bu, out_dtype=dtype, split=split)
                assert np.array_equal(_bits(swapped), _bits(want))


@pytest.mark.parametrize("stored", STORED)
def test_a_run_longer_than_the_hand_out_and_many_groups(stored):
    kn = stored == "transpose"
    # k = 2100: 66 tiles along K, a second 64-tile hand-out at split 1; a 35-row group has a second chunk
    count, n, k, rows = 2, 40, 2100, (0, 35, 40)
    assert -(-k // 32) == 66 > cases.HANDOUT and glu_split(40, count, n, k, 0) > 1 and cases.chunks(rows, 40).tolist() == [0, 2, 3]
    (_g, gate), (_u, up) = _experts(count, n, k, 70, stored), _experts(count, n, k, 80, stored)
    x = _x(40, k, 9)
    for dtype in (F32, BF16):
        for split in (1, 0):
            _compare(kn, x, rows, gate, up, count, n, k, "silu", None, None, dtype, split, twice=False)
    # n = 300: the chunked reduce's workgroups come in pairs, a second 256-column chunk per slot (44 columns of it in use)
    count, n, k, rows = 3, 300, 64, cases.EXACT
    assert -(-n // cases.REDUCE_COLUMNS) == 2 and cases.chunks(rows, 99)[-1] == cases.slots(99, count)
    (_g, gate), (_u, up) = _experts(count, n, k, 84, stored), _experts(count, n, k, 88, stored)
    x = _x(99, k, 10)
    bias = [torch.from_numpy(gen("normal_f32", 150 + i, (count, n))).cuda() for i in range(2)]
    for dtype in (F32, BF16):
        for split in (1, 2):
            _compare(kn, x, rows, gate, up, count, n, k, "silu", bias[0], bias[1], dtype, split, twice=False)
    # count = 300: the plan kernel's threads take two groups each, the group search bisects before its window of 64
    count, n, k = 300, 32, 64
    sizes = [(0, 1, 40)[(e * 7 + e // 3) % 3] for e in range(count)]
    rows = tuple(np.concatenate([[0], np.cumsum(sizes)]).tolist())
    T = rows[-1]
    assert count > 256 and {sizes.count(v) > 50 for v in (0, 1, 40)} == {True}
    assert cases.chunks(rows, T)[-1] == sizes.count(1) + 2 * sizes.count(40) <= cases.slots(T, count)
    (_g, gate), (_u, up) = _experts(count, n, k, 90, stored), _experts(count, n, k, 95, stored)
    x = _x(T, k, 11)
    bias = [torch.from_numpy(gen("normal_f32", 160 + i, (count, n))).cuda() for i in range(2)]
    for dtype in (F32, BF16):
        for split in (1, 2, 0):
            _compare(kn, x, rows, gate, up, count, n, k, "silu", bias[0], bias[1], dtype, split, twice=False)


# ----------------------------------------------------------------------------- guards

GUARD_ROWS = (0, 66, 66, 98, 99, 140)                     # groups of 66 (three chunks), 0, 32, 1 and 41 rows
GT = GUARD_ROWS[-1]


def _guarded(kn, stored, rows=GUARD_ROWS, gate_kw=None, up_kw=None, compare=True):
    """The chunked entry against the walking one on the same broken operands, splits 1, 2 and 0, NaN rows behind X, sentinels behind Y
    and the workspace."""
    (_g, gate), (_u, up) = _experts(COUNT, N, K, 30, stored), _experts(COUNT, N, K, 40, stored)

    def broken(t, kw):
        arena, maps, offs, bases = t
        kw = kw or {}
        return kw.get("arena", arena), kw.get("maps", maps), offs, kw.get("bases", bases)

    gate, up = broken(gate, gate_kw), broken(up, up_kw)
    xbuf = torch.full((GT + 16, K), float("nan"), dtype=BF16, device="cuda")
    xbuf[:GT] = _x(GT, K, 13)
    bias = [torch.from_numpy(gen("normal_f32", 60 + i, (COUNT, N)) * 20).cuda() for i in range(2)]
    outs = []
    for split in (1, 2, 0):
        for dtype in (F32, BF16):
            if compare:
                outs.append(_compare(kn, xbuf[:GT], rows, gate, up, COUNT, N, K, "silu", bias[0], bias[1], dtype, split, twice=False))
                continue
            got = _sentinels(GT + 2, N + 5, dtype)
            ws, buf = _workspace(_size(kn)(GT, COUNT, N, K, split))
            _chunked(kn)(xbuf[:GT], _rows(rows), gate, up, COUNT, N, bias_gate=bias[0], bias_up=bias[1], out_dtype=dtype, out=got[:GT, :N], split=split,
                         workspace=ws)
            torch.cuda.synchronize()
            assert _whole(buf), "bytes behind the workspace were written"
            pad = got.view(torch.uint8).view(GT + 2, -1)
            width = N * (2 if dtype == BF16 else 4)
            assert bool((pad[GT:] == SENTINEL).all()) and bool((pad[:, width:] == SENTINEL).all()), "bytes around y were written"
            assert bool((pad[:GT][torch.from_numpy(~_covered(rows, GT)).cuda()] == SENTINEL).all()), "a row of no group was written"
            outs.append(got[:GT, :N])
    assert bool(torch.isnan(xbuf[GT:].float()).all())
    return outs


@pytest.mark.parametrize("stored", STORED)
def test_broken_streams_and_tables_read_as_the_walking_entry_reads_them(stored):
    kn = stored == "transpose"
    (_g, gate), (_u, up) = _experts(COUNT, N, K, 30, stored), _experts(COUNT, N, K, 40, stored)
    whole = _guarded(kn, stored)
    # the gate arena 64 bytes short of its last expert's last tile: the buffer stays whole, packed_bytes says otherwise
    short = _guarded(kn, stored, gate_kw={"arena": gate[0][: gate[0].numel() - 64]})
    # up expert 2's stream ends one unit early by its own bases
    bases = up[3].clone()
    bases[3] -= 1
    cut = _guarded(kn, stored, up_kw={"bases": bases})
    # map codes that are no format, in the gate of expert 4 and the up of expert 0
    gm, um = gate[1].clone(), up[1].clone()
    gm.view(COUNT, -1)[4, 3] = 4
    um.view(COUNT, -1)[0, 13] = -1
    codes = _guarded(kn, stored, gate_kw={"maps": gm}, up_kw={"maps": um})
    for other in (short, cut, codes):                     # each guard changed something, and only inside its expert's rows
        assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(other, whole))
    for a, b in zip(codes, whole):
        assert np.array_equal(_bits(a[66:99]), _bits(b[66:99]))      # experts 2 and 3 are untouched by the codes of 0 and 4
    assert np.array_equal(up[3].cpu().numpy(), _experts(COUNT, N, K, 40, stored)[1][3].cpu().numpy())


BAD_ROWS = {
    "decreasing": ([0, 66, 66, 98, 50, 50], True),
    "past-T": ([0, 66, 66, 98, 99, GT + 9], True),
    "negative": ([-5, 66, 66, 98, 99, GT], True),
    "overlapping": ([0, GT, 0, GT, 0, GT], False),        # 15 chunks for 9 slots: chunks are left out, the rows are unspecified - inside y
}


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("name", list(BAD_ROWS))
def test_group_rows_are_clamped_before_any_use(name, stored):
    rows, compare = BAD_ROWS[name]
    if not compare:
        assert cases.chunks(rows, GT)[-1] > cases.slots(GT, COUNT)
    _guarded(stored == "transpose", stored, rows=rows, compare=compare)


# ----------------------------------------------------------------------------- gather

@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("k", (128, 40, 300))
def test_the_chunked_gather_is_dispatch_then_the_walking_glu_and_the_walking_gather(k, stored):
    kn = stored == "transpose"
    n = HIDDEN
    (_g, gate), (_u, up) = _experts(COUNT, n, k, 30, stored), _experts(COUNT, n, k, 40, stored)
    bias = [torch.from_numpy(gen("normal_f32", 60 + i, (COUNT, n)) * 20).cuda() for i in range(2)]
    for T, topk in GATHER_ROUTINGS:
        S = T * topk
        ids = _routing(T, topk, 100 * T + topk)
        group_rows, _row_of, src = _want_plan(ids, COUNT)
        sizes, R = np.diff(group_rows), int(group_rows[-1])
        assert 38 <= sizes.max() <= 70 and sizes[1] == 0 and sizes[3] == 0 and R < S      # a second chunk, two empty experts, dropped ids
        assert cases.chunks(group_rows, S)[2] > 0                                          # the hot group starts behind expert 0's chunk
        plan = packed.moe_plan(torch.from_numpy(ids).cuda(), COUNT)
        hand = src.copy()
        at = [0, 3, int(group_rows[2]) + 1, int(group_rows[2]) + 33, R - 1]
        hand[at] = [-1, S, I32_MIN, I32_MAX, S + 5]
        assert all(a < R for a in at) and int(group_rows[2]) + 33 < int(group_rows[3])      # one of them in a second chunk
        views = _x_views(T, k, k + T)
        assert [x_vec(v.data_ptr(), v.stride(0)) for v in views] == [k % 8 == 0, True, False]
        for src_np in (src, hand):
            src_d = torch.from_numpy(src_np).cuda()
            for vi, x in enumerate(views):
                for split in (0, 1, 2, 3):
                    need = hb.moe_glu_gather_workspace_bytes(S, COUNT, n, k, split, kn=kn, kernel="chunks")
                    assert need == cases.plan_bytes(COUNT) + hb.moe_glu_gather_workspace_bytes(S, COUNT, n, k, split, kn=kn)
                    out_dtype = F32 if (vi + split) % 2 else BF16
                    bg, bu = (bias[0], bias[1]) if split in (0, 3) else (None, None)
                    xs = hb.moe_dispatch(x, src_d, topk)
                    want = _sentinels(S + 2, n + 5, out_dtype)
                    _walk(kn)(xs, plan.group_rows, gate, up, COUNT, n, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, out=want[:S, :n], split=split)
                    walk = _sentinels(S + 2, n + 5, out_dtype)
                    hb.moe_glu_gather(x, src_d, topk, plan.group_rows, gate, up, COUNT, n, bias_gate=bg, bias_up=bu, out_dtype=out_dtype,
                                      out=walk[:S, :n], split=split, kn=kn)
                    got = _sentinels(S + 2, n + 5, out_dtype)
                    ws, buf = _workspace(need)
                    hb.moe_glu_gather(x, src_d, topk, plan.group_rows, gate, up, COUNT, n, bias_gate=bg, bias_up=bu, out_dtype=out_dtype,
                                      out=got[:S, :n], split=split, workspace=ws, kn=kn, kernel="chunks")
                    case = (T, topk, vi, split, str(out_dtype), src_np is hand)
                    assert np.array_equal(_bits(got), _bits(want)), (case, np.argwhere(_bits(got) != _bits(want))[:4])
                    assert np.array_equal(_bits(got), _bits(walk)), case
                    assert _whole(buf), "bytes behind the workspace were written"
                    assert bool((got.view(torch.uint8).view(S + 2, -1)[R:] == SENTINEL).all()), "a row of no group was written"


# ----------------------------------------------------------------------------- combine

@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("n", (8, 72, 200, 300))
def test_the_chunked_down_projection_with_the_combine_is_the_walking_one(n, stored):
    kn = stored == "transpose"
    k, T = HIDDEN, 7
    _pts, arena = _experts(COUNT, n, k, 50, stored)
    assert -(-n // cases.REDUCE_COLUMNS) == (2 if n == 300 else 1)                           # the reduce's second 256-column chunk
    for topk in (1, 2, 3, 5, 8, 9):
        S = T * topk
        ids, h_np, w_np, base_np = _combine_inputs(topk, n, 10 * n + topk)
        group_rows, row_of, _src = _want_plan(ids, COUNT)
        R = int(group_rows[-1])
        assert 0 < R < S
        plan = packed.moe_plan(torch.from_numpy(ids).cuda(), COUNT)
        h_np = h_np.copy()
        own = row_of.reshape(T, topk)[1]
        h_np[own[own >= 0]] = 0.0                         # token 1: every expert row it owns is zero, under a -0.0 base
        h_np[R:] = np.float32(np.nan)
        h = torch.from_numpy(_bf16_words_any(h_np)).cuda().view(BF16)
        hand = row_of.copy()
        live = np.flatnonzero(row_of >= 0)
        bad = [S, I32_MIN, I32_MAX, S + 5][: max(1, min(4, live.size - 2))]
        hand[live[2: 2 + len(bad)] if live.size > 2 + len(bad) else live[:len(bad)]] = bad
        w = torch.from_numpy(w_np).cuda()
        bases = (None, torch.from_numpy(base_np).cuda().to(BF16), torch.from_numpy(base_np).cuda())
        for ri, rows_np in enumerate((row_of, hand)):
            rows_d = torch.from_numpy(rows_np).cuda()
            for split in (0, 1, 2, 3):
                eff = down_split(S, COUNT, n, k, split)
                need = hb.moe_down_combine_workspace_bytes(S, COUNT, n, k, split, kn=kn, kernel="chunks")
                assert need == cases.plan_bytes(COUNT) + (eff * S * n * 4 + 15) // 16 * 16
                for expert_dtype in (F32, BF16):
                    for out_dtype in (F32, BF16):
                        for bi, base in enumerate(bases):
                            if (ri or split in (1, 3)) and bi != (split + ri) % 3:
                                continue
                            pitch = (n + 8 - n % 8 if n % 8 else n + 8, n + 3)[(bi + split) % 2]
                            want, got = _sentinels(T + 1, pitch, out_dtype), _sentinels(T + 1, pitch, out_dtype)
                            kw = dict(base=base, expert_dtype=expert_dtype, out_dtype=out_dtype, split=split, kn=kn)
                            hb.moe_down_combine(h, plan.group_rows, *arena, COUNT, n, rows_d, w, out=want[:T, :n], **kw)
                            ws, buf = _workspace(need)    # 0xFF: NaN words
                            hb.moe_down_combine(h, plan.group_rows, *arena, COUNT, n, rows_d, w, out=got[:T, :n], workspace=ws, kernel="chunks", **kw)
                            case = (topk, ri, split, str(expert_dtype), str(out_dtype), bi, pitch)
                            assert np.array_equal(_bits(got), _bits(want)), (case, np.argwhere(_bits(got) != _bits(want))[:4])
                            assert _whole(buf), "bytes behind the workspace were written"
                            assert not np.isnan(got[:T, :n].float().cpu().numpy()).any(), case


# ----------------------------------------------------------------------------- the layer and the modules

@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("route", packed.MOE_DECODE_ROUTES)
@pytest.mark.parametrize("T,topk,decode_max_rows", ((3, 2, 64), (32, 8, 256), (130, 8, 256)))
def test_the_layer_with_chunks_is_the_default_layer(T, topk, decode_max_rows, route, stored):
    kn = stored == "transpose"
    x, ids, w, base = _layer_inputs(T, topk, T == 32, 7 * T + topk)
    group_rows, _row_of, _src = _want_plan(ids, COUNT)
    assert (T * topk <= decode_max_rows) == (T != 130) and (T != 32 or np.diff(group_rows).max() > cases.CHUNK)
    w_d, ids_d = torch.from_numpy(w).cuda(), torch.from_numpy(ids).cuda()
    based = torch.from_numpy(base).cuda().to(BF16)
    experts = layer_experts(stored, "hip")
    for expert_dtype in ("float32", "bfloat16"):
        for out_dtype in ("bfloat16", "float32"):
            kw = dict(out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=decode_max_rows, stored=stored, max_tokens=1, decode_route=route)
            default, chunks = packed.PackedMoE(*experts, **kw), packed.PackedMoE(*experts, decode_grouped_kernel="chunks", **kw)
            assert default.decode_grouped_kernel == "walk" and chunks.experts.decode_grouped_kernel == "chunks"
            if route == "fused":
                assert chunks._fused_workspace.numel() == max(
                    hb.moe_glu_gather_workspace_bytes(decode_max_rows, COUNT, HIDDEN, K_IN, kn=kn, kernel="chunks"),
                    hb.moe_down_combine_workspace_bytes(decode_max_rows, COUNT, K_OUT, HIDDEN, kn=kn, kernel="chunks"))
                assert chunks._fused_workspace.numel() > default._fused_workspace.numel()
            for b in (None, based):
                got, want = chunks(x, ids_d, w_d, base=b), default(x, ids_d, w_d, base=b)
                assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (expert_dtype, out_dtype, b is None)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode is a prototype feature")
@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("route", packed.MOE_DECODE_ROUTES)
def test_a_forward_with_chunks_reads_nothing_back(route, stored):
    x, ids, w, base = _layer_inputs(8, 4, False, 5)
    ids_d, w_d, based = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(base).cuda().to(BF16)
    moe = packed.PackedMoE(*layer_experts(stored, "hip"), decode_max_rows=64, max_tokens=8, stored=stored, decode_route=route,
                           decode_grouped_kernel="chunks")
    want = _bits(packed.PackedMoE(*layer_experts(stored, "hip"), decode_max_rows=64, max_tokens=8, stored=stored, decode_route=route)(x, ids_d, w_d, base=based))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = moe(x, ids_d, w_d, base=based)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(_bits(got), want)


@pytest.mark.parametrize("stored", STORED)
def test_the_experts_mlp_with_chunks_keeps_one_workspace(monkeypatch, stored):
    kn = stored == "transpose"
    gates, ups, downs = layer_experts(stored, "hip")
    cls = packed.PackedExpertsMatmulMLP if kn else packed.PackedExpertsMLP
    T = 200
    x = _x(T, K_IN, 17)
    default, mod = cls(gates, ups, downs, decode_max_rows=T), cls(gates, ups, downs, decode_max_rows=T, decode_grouped_kernel="chunks")
    down_size = hb.packed_matmul_skinny_grouped_chunked_workspace_bytes if kn else hb.packed_linear_skinny_grouped_chunked_workspace_bytes
    assert mod._decode_workspace.numel() == max(_size(kn)(T, COUNT, HIDDEN, K_IN), down_size(T, COUNT, K_OUT, HIDDEN))
    kept = mod._decode_workspace.data_ptr()

    def never(*a, **kw):
        raise AssertionError("the chunked module called a walking binding")

    with monkeypatch.context() as mp:
        mp.setattr(hb, "packed_glu_matmul_skinny_grouped" if kn else "packed_glu_skinny_grouped", never)
        mp.setattr(hb, "packed_matmul_skinny_grouped" if kn else "packed_linear_skinny_grouped", never)
        got = [mod(x, _rows(cases.HOT)), mod(x[:5], _rows([0, 1, 1, 3, 4, 5])), mod(x, _rows(cases.HOT)),
               mod(x, torch.zeros(COUNT + 1, dtype=torch.int32, device="cuda"))]
    want = [default(x, _rows(cases.HOT)), default(x[:5], _rows([0, 1, 1, 3, 4, 5]))]
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(_bits(got[2]), _bits(want[0])) and tuple(got[3].shape) == (T, K_OUT) and not bool(got[3].any())
    assert mod._decode_workspace.data_ptr() == kept
