"""The lazy route's early form end to end (GreedyPipeline): whatever the cutoff — 0, half of what the batch needs, exactly that, every
tile — the maps, counts and columns are those of the whole-record pipeline (MTQ_LAZY=0) and the maps the oracle's; the listed launch gets
exactly the last pass's candidates ranked at or above the cutoff (none at all when the prediction is complete: the last pass still runs);
and the policy's cutoff follows the previous batch of the key.

Two batches of 128 tiles per tensor: 6 x 256x512 and 2 x 128x1024, N(0, 0.02^2) at pcc >= 0.999 — some tiles reach the last pass, most
do not.  The whole-record results and the oracle's maps are computed once."""
import math

import numpy as np
import pytest

from oracle import mtq_oracle as orc
from quantization_analysis_amd import hip_backend as hb

ALL = ["bf16", "bfp8", "bfp4", "bfp2"]
THR, SEED, TILES = 0.999, 4242, 128
SHAPES = {"6x256x512": (6, 256, 512), "2x128x1024": (2, 128, 1024)}
_CACHE = {}


def _host_inputs(name, variant=0):
    """float32 values that are exact in bf16; variant 1 has heavier tails (cubed normals): another fraction of the tiles reaches the last pass"""
    rng = np.random.default_rng(11 + variant)
    x = rng.standard_normal(SHAPES[name]).astype(np.float32)
    x = (x ** 3 if variant else x) * np.float32(0.02)
    return ((x.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)


def _inputs(name, variant=0):
    import torch

    key = ("x", name, variant)
    if key not in _CACHE:
        _CACHE[key] = torch.from_numpy(_host_inputs(name, variant)).to(torch.bfloat16).cuda()
    return _CACHE[key]


def _run(xs, monkeypatch, lazy, **hooks):
    from quantization_analysis_amd.pipeline import GreedyPipeline
    from quantization_analysis_amd.settings import settings

    monkeypatch.setenv("MTQ_LAZY", "1" if lazy else "0")
    monkeypatch.setenv("MTQ_K1_TWO_LAUNCH", "1" if lazy else "0")
    monkeypatch.setenv("MTQ_EARLY", "1")
    settings(refresh=True)
    try:
        with GreedyPipeline(ALL, "pcc", THR, SEED, chunk=4, workers=2) as pipe:
            for k, v in hooks.items():
                setattr(pipe, k, v)
            res = pipe.run(xs)
            assert pipe.host_fallbacks == 0
            return res, pipe.listed_tiles, pipe.early_tiles
    finally:
        monkeypatch.undo()
        settings(refresh=True)


def _reference(name, monkeypatch, variant=0):
    """→ (whole-record pipeline's results, oracle maps) of the batch, once"""
    key = ("ref", name, variant)
    if key not in _CACHE:
        xs = _inputs(name, variant)
        res, _listed, _early = _run(xs, monkeypatch, lazy=False)
        maps = [orc.greedy(x, ALL, "pcc", THR, SEED)[0] for x in _host_inputs(name, variant)]
        _CACHE[key] = (res, maps)
    return _CACHE[key]


def _same(got, want):
    for a, b in zip(got, want):
        assert np.array_equal(a.assignment, b.assignment) and a.counts == b.counts
        assert np.array_equal(np.array([a.pcc, a.mae, a.atol]).view(np.uint64), np.array([b.pcc, b.mae, b.atol]).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_cutoff_gives_the_whole_record_pipelines_results(name, monkeypatch):
    assert hb.early_bound()
    xs = _inputs(name)
    want, maps = _reference(name, monkeypatch)
    rank = hb.early_rank_host(SEED, TILES).astype(np.int64)
    # the last pass's candidates: the tiles that accepted bfp4 — they end in bfp4 or bfp2
    cand = [np.flatnonzero(np.isin(m.ravel(), (2, 3))) for m in maps]
    n_cand = sum(c.size for c in cand)
    assert all(0 < c.size < TILES for c in cand)
    needed = max(int(rank[c].max()) + 1 for c in cand)
    for cutoff in (0, needed // 2, needed, TILES):
        got, listed, early = _run(xs, monkeypatch, lazy=True, early_force=cutoff)
        _same(got, want)
        for r, m in zip(got, maps):
            assert np.array_equal(r.assignment, m)
        expect = sum(int((rank[c] >= cutoff).sum()) for c in cand)
        assert listed == expect, (cutoff, listed, expect)
        assert early == (n_cand - expect if cutoff else 0)
    assert expect == 0                                                   # (cutoff T: nothing was left for the list)
    assert 0 < sum(int((rank[c] >= needed // 2).sum()) for c in cand) < n_cand


@pytest.mark.gpu
def test_the_policys_cutoff_follows_the_previous_batch(monkeypatch):
    from quantization_analysis_amd.pipeline import GreedyPipeline
    from quantization_analysis_amd.settings import settings

    name = "6x256x512"
    x1, x2 = _inputs(name), _inputs(name, 1)
    want1, maps1 = _reference(name, monkeypatch)
    want2, maps2 = _reference(name, monkeypatch, 1)
    largest = [max(int(np.isin(m, (2, 3)).sum()) for m in maps) for maps in (maps1, maps2)]
    assert largest[0] != largest[1]                                      # another candidate fraction
    monkeypatch.setenv("MTQ_EARLY", "1")
    monkeypatch.setenv("MTQ_EARLY_MARGIN", "0.02")
    settings(refresh=True)
    try:
        with GreedyPipeline(ALL, "pcc", THR, SEED, chunk=4, workers=2) as pipe:
            pol = pipe.early_cutoff
            now = lambda: pol.cutoff(TILES, ALL, "pcc", THR, [SEED])
            cap = int(pipe.lazy_max_listed * TILES)
            assert now() == 0
            _same(pipe.run(x1), want1)
            assert pipe.early_tiles == 0                                 # the key's first batch is unpredicted
            assert now() == min(math.ceil(largest[0] * (1.0 + 0.02)), cap) > 0
            listed_before = pipe.listed_tiles
            _same(pipe.run(x2), want2)
            n_cand2 = sum(int(np.isin(m, (2, 3)).sum()) for m in maps2)
            assert pipe.early_tiles > 0 and pipe.early_tiles + (pipe.listed_tiles - listed_before) == n_cand2
            assert now() == min(math.ceil(largest[1] * (1.0 + 0.02)), cap)
            # another seed is another key: unpredicted
            assert pol.cutoff(TILES, ALL, "pcc", THR, [SEED + 1]) == 0
    finally:
        monkeypatch.undo()
        settings(refresh=True)


@pytest.mark.gpu
def test_ranks_are_drawn_for_an_orders_entry_made_off_the_early_route(monkeypatch):
    """The shared orders of a key may first be drawn by a batch that cannot use ranks; the first batch that can draws them then."""
    from quantization_analysis_amd.pipeline import GreedyPipeline
    from quantization_analysis_amd.settings import settings

    name = "2x128x1024"
    xs = _inputs(name)
    want, _maps = _reference(name, monkeypatch)
    monkeypatch.setenv("MTQ_EARLY", "1")
    settings(refresh=True)
    try:
        with GreedyPipeline(ALL, "pcc", THR, SEED, chunk=4, workers=2) as pipe:
            pipe.early = False
            _same(pipe.run(xs), want)
            assert all(entry[2] is None for entry in pipe._orders_cache.values())
            pipe.early, pipe.early_force = True, 12
            _same(pipe.run(xs), want)
            assert pipe.early_tiles > 0 and all(entry[2] is not None for entry in pipe._orders_cache.values())
    finally:
        monkeypatch.undo()
        settings(refresh=True)
