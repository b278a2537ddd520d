"""GPU: the MoE decode entries without the staging copies (include/mtq_moe_decode.h) and PackedMoE(decode_route="fused") on them.

Every comparison is bit equality against the STAGED route - mtq_moe_dispatch + the grouped skinny GLU, the grouped skinny product +
mtq_moe_combine, PackedMoE(decode_route="staged") - which is made of entries this file's subject does not touch; the layer is held to
the NumPy float32 combine of tests/moe_cases.py over the staged experts' rows as well.  Where a shape is there to reach a path (a
second 32-row chunk, the element-wise X loads, an effective split above 1, a second 256-column chunk of the reduce), the test
derives the path from the shape with the host arithmetic (tests/moe_fused_cases.py) and asserts it.

  gather    5 experts of k → 96 in both orientations, k = 128, 40 (two tiles, the second cut by K) and 300 (no 16-byte rows); topk 1, 2,
            3, 8; a routing with a 33-70 row group (a second, short chunk), two empty experts, a token one expert names twice and
            dropped ids; x contiguous, a view of a wider buffer, and starting at an odd element; NaN rows behind x; split 0 .. 3; both
            output types; with and without biases; a hand-made src with -1, S, S + 5 and the int32 extremes inside a group's rows; a
            workspace of 0xFF bytes; y a pitched view of sentinels with sentinel rows behind it.
  combine   5 experts of 96 → n, n = 8, 72, 200, 300 (a second 256-column chunk); topk 1, 2, 3, 5, 8, 9; split 0 .. 3;
            expert_dtype x out_dtype; no base, a bf16 base, a float32 base; a token whose rows of h are zeros with a -0.0 base; dropped
            slots; a hand-made row_of with values outside [0, S); a workspace of NaN bytes; y at an aligned and an odd pitch in sentinels.
  layer     128 → 96 → 64, both `stored`: (T, K) = (3, 2), (32, 8) with one hot expert, (130, 8) with decode_max_rows = 256 (the staged
            route inside a fused module); expert_dtype x out_dtype, with and without base, int32 and int64 ids; under torch's
            sync-debug mode "error"; forward_logits with mixtral's routing on 5 experts."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tests.inputs import gen, to_bf16_valued
from tests.moe_cases import I32_MAX, I32_MIN, SENTINEL, _bf16_valued, _bf16_words, _want_combine, _want_plan
from tests.moe_fused_cases import (CHUNK, COUNT, HIDDEN, K_IN, K_OUT, REDUCE_COLUMNS, STORED, _weights, down_split, glu_split, layer_experts,
                                   pack_experts, x_vec)

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def _bits(t) -> np.ndarray:
    t = t.detach()
    return (t.contiguous().view(torch.int16) if t.dtype == BF16 else t.contiguous().view(torch.int32)).cpu().numpy()


def _sentinels(rows, pitch, dtype):
    """A (rows, pitch) tensor of sentinel bytes: an output is a view into it, and what the call leaves alone stays sentinel."""
    return torch.full((rows * pitch * (2 if dtype == BF16 else 4),), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).view(rows, pitch)


@functools.lru_cache(maxsize=None)
def _arena(n, k, seed, stored):
    """The device arena of COUNT experts (n, k) in one orientation → hip_backend's (arena, maps, offsets, bases)."""
    batch = packed.batch_to_device(packed.as_batch(pack_experts(_weights(COUNT, n, k, seed), seed + 3, stored, backend="hip")))
    return batch.arena, batch.maps_dev, batch.offsets_dev, batch.bases_dev


def _routing(T, K, seed):
    """Expert 2 is hot (a group above 32 rows when S allows), experts 1 and 3 stay empty, some slots name experts of another rank, and
    with K > 1 token 0 names expert 4 twice."""
    pattern = np.array([2, 2, 2, 2, 2, 2, 2, 0, 4, -1, 2, 2, 2, 2, 2, 2, 2, 0, 4, COUNT + 3], dtype=np.int64)      # 7 slots in 10 on expert 2
    ids = np.random.default_rng(seed).permutation(pattern[np.arange(T * K) % pattern.size]).reshape(T, K)
    ids[0, :] = 4 if K > 1 else 2
    ids[-1, -1] = -1 if T > 1 else ids[-1, -1]
    return ids


# ----------------------------------------------------------------------------- gather

GATHER_ROUTINGS = ((70, 1), (30, 2), (20, 3), (9, 8))     # (tokens, topk): S = 70, 60, 60, 72


def _x_views(T, k, seed):
    """x (T, k) bf16 three ways, with the same words: contiguous, a pitched view of a wider buffer (16-byte rows), and from an odd
    element of a buffer on (no 16-byte rows); behind each, four rows of NaN words that no call may read."""
    words = torch.from_numpy(_bf16_words(gen("normal_f32", seed, (T, k)) * 50)).cuda().view(BF16)
    pitch = (k + 15) // 8 * 8
    views = []
    for ld, lead in ((k, 0), (pitch, 0), (k + 3, 1)):
        buf = torch.full((lead + (T + 4) * ld,), float("nan"), dtype=BF16, device="cuda")
        view = buf[lead: lead + T * ld].view(T, ld)[:, :k]
        view.copy_(words)
        views.append(view)
    return views


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("k", (128, 40, 300))
def test_the_gathered_glu_is_dispatch_then_the_grouped_skinny_glu(k, stored):
    kn = stored == "transpose"
    n = HIDDEN
    gate, up = _arena(n, k, 30, stored), _arena(n, k, 40, stored)
    staged = hb.packed_glu_matmul_skinny_grouped if kn else hb.packed_glu_skinny_grouped
    bias = [torch.from_numpy(gen("normal_f32", 60 + i, (COUNT, n)) * 20).cuda() for i in range(2)]
    tiles_k = -(-k // 32)
    for T, K in GATHER_ROUTINGS:
        S = T * K
        ids = _routing(T, K, 100 * T + K)
        group_rows, _row_of, src = _want_plan(ids, COUNT)
        sizes = np.diff(group_rows)
        R = int(group_rows[-1])
        assert 33 <= sizes.max() <= 70 and sizes.max() % CHUNK != 0, sizes          # a second chunk, and a short last one
        assert sizes[1] == 0 and sizes[3] == 0 and R < S and (K == 1 or (ids[0] == 4).all())
        plan = packed.moe_plan(torch.from_numpy(ids).cuda(), COUNT)
        assert np.array_equal(plan.src.cpu().numpy(), src)
        hand = src.copy()                                 # -1, S, S + 5 and the int32 extremes inside groups' rows: zero rows
        at = [0, 3, int(group_rows[2]) + 1, int(group_rows[2]) + 33, R - 1]
        hand[at] = [-1, S, I32_MIN, I32_MAX, S + 5]
        assert all(a < R for a in at) and len(set(at)) == 5 and int(group_rows[2]) + 33 < int(group_rows[3])      # one of them in a second chunk
        views = _x_views(T, k, k + T)
        assert [x_vec(v.data_ptr(), v.stride(0)) for v in views] == [k % 8 == 0, True, False]      # the element-wise X path is met
        for src_np in (src, hand):
            src_d = torch.from_numpy(src_np).cuda()
            for vi, x in enumerate(views):
                for split in (0, 1, 2, 3):
                    eff = glu_split(S, COUNT, n, k, split)
                    assert eff == (min(split, tiles_k) if split else eff) and (split < 2 or eff > 1)
                    need = hb.moe_glu_gather_workspace_bytes(S, COUNT, n, k, split, kn=kn)
                    assert need == hb.packed_glu_skinny_grouped_workspace_bytes(S, COUNT, n, k, split) == (2 * eff * S * n * 4 + 15) // 16 * 16
                    for out_dtype in ((F32, BF16) if vi == 0 or split == 2 else (BF16,)):
                        for bg, bu in (((None, None), (bias[0], bias[1])) if split in (0, 3) else ((None, None),)):
                            xs = hb.moe_dispatch(x, src_d, K)
                            assert xs.is_contiguous() and tuple(xs.shape) == (S, k)
                            want = _sentinels(S + 2, n + 5, out_dtype)
                            staged(xs, plan.group_rows, gate, up, COUNT, n, bias_gate=bg, bias_up=bu, out_dtype=out_dtype, out=want[:S, :n], split=split)
                            got = _sentinels(S + 2, n + 5, out_dtype)
                            ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
                            y = hb.moe_glu_gather(x, src_d, K, plan.group_rows, gate, up, COUNT, n, bias_gate=bg, bias_up=bu, out_dtype=out_dtype,
                                                  out=got[:S, :n], split=split, workspace=ws[:need], kn=kn)
                            assert y.data_ptr() == got.data_ptr()
                            case = (T, K, vi, split, str(out_dtype), bg is not None, src_np is hand)
                            assert np.array_equal(_bits(got), _bits(want)), (case, np.argwhere(_bits(got) != _bits(want))[:4])
                            assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
                            pad = got.view(torch.uint8).view(S + 2, -1)
                            assert bool((pad[R:] == SENTINEL).all()), "a row of no group was written"


def test_the_gathered_glu_module_functions():
    """packed.moe_glu on the device plan against moe_dispatch + glu_grouped_skinny, both `stored`, from the batches as the module holds them."""
    T, K = 9, 8
    ids = torch.from_numpy(_routing(T, K, 5)).cuda()
    x = torch.from_numpy(_bf16_words(gen("normal_f32", 3, (T, K_IN)) * 50)).cuda().view(BF16)
    for stored in STORED:
        gates, ups, _downs = layer_experts(stored, "hip")
        plan = packed.moe_plan(ids, COUNT)
        glu = packed.glu_grouped_skinny if stored == "rows" else packed.glu_matmul_grouped_skinny
        for out_dtype in ("bfloat16", "float32"):
            for split in (0, 2):
                want = glu(packed.moe_dispatch(x, plan), plan.group_rows, gates, ups, out_dtype=out_dtype, split=split)
                got = packed.moe_glu(x, plan, gates, ups, out_dtype=out_dtype, stored=stored, split=split)
                assert np.array_equal(_bits(got), _bits(want)), (stored, out_dtype, split)


# ----------------------------------------------------------------------------- combine

COMBINE_TOKENS = 7


def _combine_inputs(K, n, seed):
    """(ids, h words, weights, base) for COMBINE_TOKENS tokens: the rows of h that token 1's slots own are zeros and its base is -0.0."""
    T = COMBINE_TOKENS
    rng = np.random.default_rng(seed)
    ids = _routing(T, K, seed)
    ids[1, 0] = 0                                         # token 1 has a live slot
    w = rng.standard_normal((T, K)).astype(np.float32)
    w[rng.random((T, K)) < 0.15] = 0.0
    w[1, 0] = -0.5                                        # -0.5 * +0 = -0, and -0.0 + -0 stays -0
    h = _bf16_valued(rng.standard_normal((T * K, HIDDEN)).astype(np.float32))
    base = _bf16_valued(rng.standard_normal((T, n)).astype(np.float32))
    base[1] = -0.0
    return ids, h, w, base


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("n", (8, 72, 200, 300))
def test_the_down_projection_with_the_combine_is_the_grouped_product_then_combine(n, stored):
    kn = stored == "transpose"
    k, T = HIDDEN, COMBINE_TOKENS
    arena = _arena(n, k, 50, stored)
    staged = hb.packed_matmul_skinny_grouped if kn else hb.packed_linear_skinny_grouped
    nchunks = -(-n // REDUCE_COLUMNS)
    assert nchunks == (2 if n == 300 else 1)              # the reduce's second 256-column chunk
    for K in (1, 2, 3, 5, 8, 9):
        S = T * K
        ids, h_np, w_np, base_np = _combine_inputs(K, n, 10 * n + K)
        group_rows, row_of, _src = _want_plan(ids, COUNT)
        R = int(group_rows[-1])
        assert 0 < R < S                                  # dropped slots
        plan = packed.moe_plan(torch.from_numpy(ids).cuda(), COUNT)
        assert np.array_equal(plan.row_of.cpu().numpy(), row_of)
        h_np = h_np.copy()
        own = row_of.reshape(T, K)[1]
        h_np[own[own >= 0]] = 0.0                         # token 1: every expert row it owns is zero
        h_np[R:] = np.float32(np.nan)                     # rows of no group: never read
        h = torch.from_numpy(_bf16_words_any(h_np)).cuda().view(BF16)
        hand = row_of.copy()
        live = np.flatnonzero(row_of >= 0)
        bad = [S, I32_MIN, I32_MAX, S + 5][: max(1, min(4, live.size - 2))]
        hand[live[2: 2 + len(bad)] if live.size > 2 + len(bad) else live[:len(bad)]] = bad
        assert ((hand < 0) | (hand >= S)).sum() > ((row_of < 0) | (row_of >= S)).sum()
        w = torch.from_numpy(w_np).cuda()
        bases = (None, torch.from_numpy(base_np).cuda().to(BF16), torch.from_numpy(base_np).cuda())
        assert _bits(bases[1])[1].view(np.uint16).tolist() == [0x8000] * n
        for ri, rows_np in enumerate((row_of, hand)):
            rows_d = torch.from_numpy(rows_np).cuda()
            for split in (0, 1, 2, 3):
                eff = down_split(S, COUNT, n, k, split)
                assert eff == (min(split, 3) if split else eff) and (split < 2 or eff > 1)
                need = hb.moe_down_combine_workspace_bytes(S, COUNT, n, k, split, kn=kn)
                assert need == (eff * S * n * 4 + 15) // 16 * 16
                for expert_dtype in (F32, BF16):
                    ys = staged(h, plan.group_rows, *arena, COUNT, n, out_dtype=expert_dtype, split=split)
                    for out_dtype in (F32, BF16):
                        for bi, base in enumerate(bases):
                            if (ri or split in (1, 3)) and bi != (split + ri) % 3:
                                continue                  # every base at split 0 and 2 on the plan's rows, one in turn elsewhere
                            for pitch in (n + 8 - n % 8 if n % 8 else n + 8, n + 3):
                                want = _sentinels(T + 1, pitch, out_dtype)
                                hb.moe_combine(ys, rows_d, w, base=base, out_dtype=out_dtype, out=want[:T, :n])
                                got = _sentinels(T + 1, pitch, out_dtype)
                                ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")        # NaN words
                                hb.moe_down_combine(h, plan.group_rows, *arena, COUNT, n, rows_d, w, base=base, expert_dtype=expert_dtype,
                                                    out_dtype=out_dtype, out=got[:T, :n], split=split, workspace=ws[:need], kn=kn)
                                case = (K, ri, split, str(expert_dtype), str(out_dtype), bi, pitch)
                                assert np.array_equal(_bits(got), _bits(want)), (case, np.argwhere(_bits(got) != _bits(want))[:4])
                                assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
                                assert not np.isnan(got[:T, :n].float().cpu().numpy()).any(), case


def _bf16_words_any(a32: np.ndarray) -> np.ndarray:
    """_bf16_words for values that are bf16 values already, NaN included: the high halves."""
    return (np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


# ----------------------------------------------------------------------------- the layer

def _layer_inputs(T, K, hot, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(_bf16_words(gen("normal_f32", seed, (T, K_IN)) * 50)).cuda().view(BF16)
    if hot:                                               # expert 2 takes most slots: groups above 32 rows
        ids = rng.choice(np.array([0, 2, 2, 2, 2, 4, -1, COUNT], dtype=np.int64), size=(T, K))
    else:
        ids = rng.integers(0, COUNT, size=(T, K)).astype(np.int64)
    w = rng.random((T, K)).astype(np.float32) + 0.25
    base = _bf16_valued(rng.standard_normal((T, K_OUT)).astype(np.float32))
    return x, ids, w, base


@pytest.mark.parametrize("stored", STORED)
@pytest.mark.parametrize("T,K,decode_max_rows", ((3, 2, 64), (32, 8, 256), (130, 8, 256)))
def test_the_fused_layer_is_the_staged_layer(T, K, decode_max_rows, stored):
    S = T * K
    x, ids, w, base = _layer_inputs(T, K, T == 32, 7 * T + K)
    group_rows, row_of, _src = _want_plan(ids, COUNT)
    assert (S <= decode_max_rows) == (T != 130) and (T != 32 or np.diff(group_rows).max() > CHUNK)
    w_d = torch.from_numpy(w).cuda()
    experts = layer_experts(stored, "hip")
    for expert_dtype in ("float32", "bfloat16"):
        for out_dtype in ("bfloat16", "float32"):
            kw = dict(out_dtype=out_dtype, expert_dtype=expert_dtype, decode_max_rows=decode_max_rows, stored=stored, max_tokens=1)
            staged, fused = packed.PackedMoE(*experts, **kw), packed.PackedMoE(*experts, decode_route="fused", **kw)
            assert fused.backend == "hip" and fused._fused_workspace is not None and staged._fused_workspace is None
            kn = stored == "transpose"
            assert fused._fused_workspace.numel() == max(hb.moe_glu_gather_workspace_bytes(decode_max_rows, COUNT, HIDDEN, K_IN, kn=kn),
                                                         hb.moe_down_combine_workspace_bytes(decode_max_rows, COUNT, K_OUT, HIDDEN, kn=kn))
            # the staged experts' rows, for the NumPy combine
            plan = packed.moe_plan(torch.from_numpy(ids).cuda(), COUNT)      # a workspace of its own making, at S = 1040 on three kernels
            assert np.array_equal(plan.row_of.cpu().numpy(), row_of)
            ys = staged.experts(packed.moe_dispatch(x, plan), plan.group_rows).float().cpu().numpy()
            for with_base in (False, True):
                based = torch.from_numpy(base).cuda().to(BF16) if with_base else None
                with np.errstate(all="ignore"):
                    acc = _want_combine(row_of, w, ys, base if with_base else None, T, K)
                loop = acc.view(np.int32) if out_dtype == "float32" else _bf16_words(acc).reshape(T, K_OUT)
                for ids_d in (torch.from_numpy(ids).cuda(), torch.from_numpy(ids).cuda().to(torch.int32)):
                    want, got = staged(x, ids_d, w_d, base=based), fused(x, ids_d, w_d, base=based)
                    case = (expert_dtype, out_dtype, with_base, str(ids_d.dtype))
                    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (case, np.argwhere(_bits(got) != _bits(want))[:4])
                    assert np.array_equal(_bits(got), loop), (case, "the NumPy combine of the staged experts' rows")


@pytest.mark.filterwarnings("ignore:Synchronization debug mode is a prototype feature")
@pytest.mark.parametrize("stored", STORED)
def test_the_fused_forward_reads_nothing_back(stored):
    x, ids, w, base = _layer_inputs(8, 4, False, 5)
    ids_d, w_d, based = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(base).cuda().to(BF16)
    moe = packed.PackedMoE(*layer_experts(stored, "hip"), decode_max_rows=64, max_tokens=8, stored=stored, decode_route="fused")
    want = _bits(moe(x, ids_d, w_d, base=based))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = moe(x, ids_d, w_d, base=based)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(_bits(got), want)


def test_forward_logits_follows_the_decode_route():
    T = 6
    router = packed.MOE_ROUTINGS["mixtral"]               # softmax, top-2, renormalised: no groups, so 5 experts will do
    assert (router.topk, router.n_group) == (2, 1)
    x, _ids, _w, base = _layer_inputs(T, router.topk, False, 11)
    logits = torch.from_numpy(gen("normal_f32", 12, (T, COUNT)) * 100).cuda()
    based = torch.from_numpy(base).cuda().to(BF16)
    for stored in STORED:
        kw = dict(decode_max_rows=64, stored=stored, router="mixtral")
        staged, fused = packed.PackedMoE(*layer_experts(stored, "hip"), **kw), packed.PackedMoE(*layer_experts(stored, "hip"), decode_route="fused", **kw)
        for b in (None, based):
            assert np.array_equal(_bits(fused.forward_logits(x, logits, base=b)), _bits(staged.forward_logits(x, logits, base=b))), (stored, b is None)
