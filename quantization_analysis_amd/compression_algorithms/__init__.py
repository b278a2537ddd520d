"""Search algorithms selectable from the JSON config (`algorithm` key) — same names as the reference's registry
(compression_algorithms/__init__.py:11-29).  ALGORITHM_REGISTRY holds the mixed-tile family and the `none` baseline;
`mixed-tile` is the reference's alias of the greedy search.  LAYOUT_ALGORITHMS holds the reference's `transpose`
experiment: every format applied along the other axis of the weight (K1T / K2T on the hip backend), not a mixed-tile
search.  BUDGET_ALGORITHMS holds `mixed-tile-budget`, the map at a size target, which the reference
does not have: ALGORITHM_REGISTRY stays the reference's registry, name for name.  create_algorithm consults the three tables.
"""
from __future__ import annotations

from . import base as _base, config as _config
from . import mixed_tile_budget as _budget
from . import mixed_tile_greedy as _greedy, mixed_tile_random as _random, mixed_tile_threshold as _threshold, none as _none
from . import transpose as _transpose

CompressionAlgorithm, CompressionResult = _base.CompressionAlgorithm, _base.CompressionResult
CompressionConfig, load_compression_config = _config.CompressionConfig, _config.load_compression_config
NoneCompression = _none.NoneCompression
MixedTileGreedyCompression = _greedy.MixedTileGreedyCompression
MixedTileRandomCompression = _random.MixedTileRandomCompression
MixedTileThresholdCompression = _threshold.MixedTileThresholdCompression
MixedTileBudgetCompression = _budget.MixedTileBudgetCompression
TransposeCompression = _transpose.TransposeCompression

ALGORITHM_REGISTRY: dict = {cls.name: cls for cls in (NoneCompression, MixedTileGreedyCompression,
                                                      MixedTileRandomCompression, MixedTileThresholdCompression)}
ALGORITHM_REGISTRY["mixed-tile"] = MixedTileGreedyCompression
LAYOUT_ALGORITHMS: dict = {TransposeCompression.name: TransposeCompression}
BUDGET_ALGORITHMS: dict = {MixedTileBudgetCompression.name: MixedTileBudgetCompression}


def create_algorithm(name: str, params: dict | None = None) -> CompressionAlgorithm:
    """Case-insensitive lookup; an unknown name lists what is available."""
    key = name.strip().lower()
    algorithm_cls = ALGORITHM_REGISTRY.get(key) or LAYOUT_ALGORITHMS.get(key) or BUDGET_ALGORITHMS.get(key)
    if algorithm_cls is None:
        known = ", ".join(sorted({**ALGORITHM_REGISTRY, **LAYOUT_ALGORITHMS, **BUDGET_ALGORITHMS}))
        raise ValueError(f"Unsupported compression algorithm '{name}'. Supported: {known}")
    return algorithm_cls.from_params(params if params else {})
