"""The refusal ladders of the packed C entries (csrc/mtq_packed.hip), which tests/test_packed_refusals_host.py holds to the texts recorded
in tests/golden/packed_refusals.json: the twenty product entries, their fourteen size functions (every product pair but block, wide and
glu wide has one) and the eight pack / unpack entries.

An entry's ladder lists its defects in the order the entry checks them.  It makes one call per defect and one call per adjacent pair
of defects, and records (return code, mtq_last_error text) of each; a pair call has to report the earlier of the two.  Where two
defects set the same argument the earlier one's value is used.  A size function records its return value, and has a few good calls
too: it touches no device.  Every other call carries at least one defect, so nothing reaches the device check and nothing is launched,
with or without a GPU.  Pointers are fake aligned integers: none of these checks dereferences one (mtq_packed_offsets does read its
map on the host; it is not in the ladder).

Run as a script, this module writes the fixture from the library hip_backend loads (MTQ_LIB selects it):

    MTQ_LIB=/path/to/libmtq_hip.so python -m tests.packed_refusal_cases tests/golden/packed_refusals.json

Sites the ladders leave out, by name:
  skinny, glu skinny (all four entries): "too many workgroups for one launch".  blocks is at most 2 * tiles_h * split / 4 with split <=
      tiles_w, and tile_grid has already held tiles_h * tiles_w to 2^31: the guard cannot fire.
  chunked, wide grouped, glu wide grouped: the `slots` term of that guard alone; slots <= total_rows <= INT32_MAX.  The ladder reaches
      the site through `blocks`.
  every product entry: a failing launch (check_launch) and a missing device (require_device); they need a device, or its absence.
The grouped skinny and glu grouped skinny entries reach the workgroup guard only with a packed_bytes above 2^40 (count * tiles_h above
2^33 makes the arena's least size above 2^41); the ladder passes such a number, since no buffer stands behind it.
"""
from __future__ import annotations

import json
import sys

from quantization_analysis_amd import hip_backend as hb

F32, BF16 = hb.DTYPE_F32, hb.DTYPE_BF16
SILU = hb.ACT_CODE["silu"]
BLOB = 320                                     # a bfp2 tile: the least a tile takes in a stream
N, K, M, T, COUNT = 64, 96, 4, 4, 2            # a 2 x 3 tile grid; four rows; two experts
TILES = 6
BIG = 1 << 30
HUGE = 1 << 62                                 # a byte count no check finds short


def ptr(i):
    return 0x10000 * (i + 1)


def _grid(rows, cols):
    """tile_grid's refusals on (rows, cols), as argument names"""
    return [(f"{rows} = 0", {rows: 0}), (f"{cols} = 0", {cols: 0}), (f"{rows} > 2^30", {rows: BIG + 1}), (f"{cols} > 2^30", {cols: BIG + 1}),
            ("tiles > 2^31", {rows: BIG, cols: BIG})]


def _nulls(names):
    return [(f"{name} null", {name: None}) for name in names]


def _skinny_shape():
    return [("m = 0", {"m": 0}), ("m < 0", {"m": -1}), ("m = 33", {"m": 33}), ("split < 0", {"split": -1})] + _grid("n", "k")


def _grouped_shape(glu=False):
    d = [("total_rows = 0", {"total_rows": 0}), ("total_rows > INT32_MAX", {"total_rows": 1 << 31}), ("count = 0", {"count": 0}),
         ("count < 0", {"count": -1}), ("count > INT32_MAX", {"count": 1 << 31}), ("split < 0", {"split": -1})] + _grid("n", "k")
    d += [("tiles > batch max", {"n": 1 << 20, "k": 1 << 18}), ("tiles in the batch", {"n": 1 << 15, "k": 1 << 15, "count": (1 << 20) + 1}),
          ("split workspace too large", {"total_rows": (1 << 31) - 1, "n": BIG, "k": 64, "count": 1, "split": 2})]
    if glu:
        d.append(("glu workspace too large", {"total_rows": (1 << 31) - 1, "n": BIG, "k": 32, "count": 1, "split": 1}))
    return d


def _no_split(defects):
    """a shape rule's defects for an entry without a split argument: the wide grouped entries pass split 1 themselves"""
    return [(label, {a: v for a, v in over.items() if a != "split"}) for label, over in defects if "split" not in label]


def _workspace(need_with, short):
    """null, misaligned, short; need_with: the arguments under which the entry needs a workspace, short: a size just below its need"""
    ctx = dict(need_with)
    return [("workspace null", dict(ctx, workspace=None)), ("workspace misaligned", dict(ctx, workspace=ptr(40) + 8)),
            ("workspace short", dict(ctx, workspace_bytes=short))]


# ---- the entries: name -> (parameter names in C order, good values, defects in the order the entry checks them)

SINGLE = ("x", "m", "k", "ldx", "packed", "packed_bytes", "map", "offsets", "n", "bias", "y", "out_dtype", "ldy")
SINGLE_GOOD = dict(x=ptr(0), m=M, k=K, ldx=K, packed=ptr(1), packed_bytes=TILES * BLOB, map=ptr(2), offsets=ptr(3), n=N, bias=None, y=ptr(4),
                   out_dtype=F32, ldy=N, split=0, workspace=ptr(40), workspace_bytes=1 << 20, stream=None)
GLU_SINGLE = ("x", "m", "k", "ldx", "gate_packed", "gate_bytes", "gate_map", "gate_offsets", "up_packed", "up_bytes", "up_map", "up_offsets", "n",
              "bias_gate", "bias_up", "act", "y", "out_dtype", "ldy")
GLU_SINGLE_GOOD = dict(x=ptr(0), m=M, k=K, ldx=K, gate_packed=ptr(1), gate_bytes=TILES * BLOB, gate_map=ptr(2), gate_offsets=ptr(3),
                       up_packed=ptr(5), up_bytes=TILES * BLOB, up_map=ptr(6), up_offsets=ptr(7), n=N, bias_gate=None, bias_up=None, act=SILU,
                       y=ptr(4), out_dtype=BF16, ldy=N, split=0, workspace=ptr(40), workspace_bytes=1 << 20, stream=None)
GROUPED = ("x", "total_rows", "k", "ldx", "group_rows", "packed", "packed_bytes", "maps", "offsets", "bases", "count", "n", "bias", "ldb", "y",
           "out_dtype", "ldy")
GROUPED_GOOD = dict(x=ptr(0), total_rows=T, k=K, ldx=K, group_rows=ptr(8), packed=ptr(1), packed_bytes=COUNT * TILES * BLOB, maps=ptr(2),
                    offsets=ptr(3), bases=ptr(9), count=COUNT, n=N, bias=ptr(10), ldb=N, y=ptr(4), out_dtype=F32, ldy=N, split=0,
                    workspace=ptr(40), workspace_bytes=1 << 20, stream=None)
GLU_GROUPED = ("x", "total_rows", "k", "ldx", "group_rows", "gate_packed", "gate_bytes", "gate_maps", "gate_offsets", "gate_bases", "up_packed",
               "up_bytes", "up_maps", "up_offsets", "up_bases", "count", "n", "bias_gate", "bias_up", "ldb", "act", "y", "out_dtype", "ldy")
GLU_GROUPED_GOOD = dict(x=ptr(0), total_rows=T, k=K, ldx=K, group_rows=ptr(8), gate_packed=ptr(1), gate_bytes=COUNT * TILES * BLOB,
                        gate_maps=ptr(2), gate_offsets=ptr(3), gate_bases=ptr(9), up_packed=ptr(5), up_bytes=COUNT * TILES * BLOB, up_maps=ptr(6),
                        up_offsets=ptr(7), up_bases=ptr(11), count=COUNT, n=N, bias_gate=None, bias_up=ptr(10), ldb=N, act=SILU, y=ptr(4),
                        out_dtype=BF16, ldy=N, split=0, workspace=ptr(40), workspace_bytes=1 << 20, stream=None)

BAD_DTYPE = [("out_dtype", {"out_dtype": 7})]
PITCHES = [("ldx < k", {"ldx": K - 1}), ("ldy < n", {"ldy": N - 1})]
BAD_ACT = [("act", {"act": 2})]
PLAN = 16                                      # the grouped plan of COUNT = 2 groups: 3 int32, rounded to 16
# The grid rungs of the entries with a split keep two tile columns (k = 64): when the rung before sets split 2, its workspace is still needed.


def _linear_args(packed="packed", nbytes="packed_bytes", pointers=("x", "packed", "map", "offsets", "y")):
    return (_nulls(pointers) + BAD_DTYPE + [("m = 0", {"m": 0}), ("m < 0", {"m": -1})] + _grid("n", "k") + PITCHES + [("m > 2^40", {"m": (1 << 40) + 1})]
            + [(f"{packed} misaligned", {packed: ptr(1) + 8}), (f"{nbytes} short", {nbytes: TILES * BLOB - 1})])


def _block_like(grid_m, grid_n):
    return _linear_args() + [("grid > INT32_MAX", {"m": grid_m, "n": grid_n, "k": 32, "ldx": 32, "ldy": grid_n, "packed_bytes": (grid_n // 32) * BLOB})]


def _glu_wide():
    gate = _linear_args("gate_packed", "gate_bytes", ("x", "gate_packed", "gate_map", "gate_offsets", "y"))
    up = _nulls(("up_packed", "up_map", "up_offsets")) + [("up_packed misaligned", {"up_packed": ptr(5) + 8}), ("up_bytes short", {"up_bytes": TILES * BLOB - 1})]
    n = 1 << 20
    return gate + up + BAD_ACT + [("grid > INT32_MAX", {"m": BIG, "n": n, "k": 32, "ldx": 32, "ldy": n, "gate_bytes": (n // 32) * BLOB, "up_bytes": (n // 32) * BLOB})]


def _skinny():
    ws = M * N * 4                                   # one slice's partial sums
    return (_nulls(("x", "packed", "map", "offsets", "y")) + BAD_DTYPE + _skinny_shape() + PITCHES
            + [("packed misaligned", {"packed": ptr(1) + 8}), ("packed_bytes short", {"packed_bytes": TILES * BLOB - 1})]
            + _workspace({"split": 2}, 2 * ws - 1))


def _glu_skinny():
    ws = 2 * M * N * 4                               # both projections, at every split
    return (_nulls(("x", "gate_packed", "gate_map", "gate_offsets", "up_packed", "up_map", "up_offsets", "y")) + BAD_DTYPE + _skinny_shape() + PITCHES
            + [("gate_packed misaligned", {"gate_packed": ptr(1) + 8}), ("up_packed misaligned", {"up_packed": ptr(5) + 8}),
               ("gate_bytes short", {"gate_bytes": TILES * BLOB - 1}), ("up_bytes short", {"up_bytes": TILES * BLOB - 1})]
            + BAD_ACT + _workspace({}, ws - 1) + [("workspace short at split 2", {"split": 2, "workspace_bytes": 2 * ws - 1})])


GROUPED_POINTERS = ("x", "group_rows", "packed", "maps", "offsets", "bases", "y")
GROUPED_STREAM = [("ldb < n", {"ldb": N - 1}), ("packed misaligned", {"packed": ptr(1) + 8}), ("packed_bytes short", {"packed_bytes": COUNT * TILES * BLOB - 1})]


def _skinny_grouped():
    n = 1 << 20                                      # count * tiles_h = 2^21 * 2^15 = 2^36 waves
    return (_nulls(GROUPED_POINTERS) + BAD_DTYPE + _grouped_shape() + PITCHES + GROUPED_STREAM + _workspace({"split": 2}, 2 * T * N * 4 - 1)
            + [("grid > INT32_MAX", {"total_rows": 1, "count": 1 << 21, "n": n, "k": 64, "ldx": 64, "ldy": n, "ldb": n, "packed_bytes": HUGE})])


def _chunked():
    n = 1 << 15                                      # slots 2^26, tiles_h 2^10
    return (_nulls(GROUPED_POINTERS) + BAD_DTYPE + _grouped_shape() + PITCHES + GROUPED_STREAM + _workspace({}, PLAN - 1)
            + [("workspace short at split 2", {"split": 2, "workspace_bytes": PLAN + 2 * T * N * 4 - 1}),
               ("grid > INT32_MAX", {"total_rows": (1 << 31) - 1, "count": 1, "n": n, "k": 64, "ldx": 64, "ldy": n, "packed_bytes": 2 * (n // 32) * BLOB})])


def _wide_grouped():
    n = 1 << 20                                      # slots 2^24, 2^13 column blocks
    return (_nulls(GROUPED_POINTERS) + BAD_DTYPE + _no_split(_grouped_shape()) + PITCHES + GROUPED_STREAM + _workspace({}, PLAN - 1)
            + [("grid > INT32_MAX", {"total_rows": (1 << 31) - 1, "count": 1, "n": n, "k": 32, "ldx": 32, "ldy": n, "packed_bytes": (n // 32) * BLOB})])


GLU_GROUPED_POINTERS = ("x", "group_rows", "gate_packed", "gate_maps", "gate_offsets", "gate_bases", "up_packed", "up_maps", "up_offsets", "up_bases", "y")
GLU_GROUPED_STREAM = [("ldb < n", {"ldb": N - 1}), ("gate_packed misaligned", {"gate_packed": ptr(1) + 8}), ("up_packed misaligned", {"up_packed": ptr(5) + 8}),
                      ("gate_bytes short", {"gate_bytes": COUNT * TILES * BLOB - 1}), ("up_bytes short", {"up_bytes": COUNT * TILES * BLOB - 1})]


def _glu_wide_grouped():
    n = 1 << 20
    return (_nulls(GLU_GROUPED_POINTERS) + BAD_DTYPE + _no_split(_grouped_shape()) + PITCHES + GLU_GROUPED_STREAM + BAD_ACT + _workspace({}, PLAN - 1)
            + [("grid > INT32_MAX", {"total_rows": (1 << 31) - 1, "count": 1, "n": n, "k": 32, "ldx": 32, "ldy": n, "gate_bytes": (n // 32) * BLOB,
                                     "up_bytes": (n // 32) * BLOB})])


def _glu_skinny_grouped():
    n, ws = 1 << 20, 2 * T * N * 4
    return (_nulls(GLU_GROUPED_POINTERS) + BAD_DTYPE + _grouped_shape(glu=True) + PITCHES + GLU_GROUPED_STREAM + BAD_ACT + _workspace({}, ws - 1)
            + [("workspace short at split 2", {"split": 2, "workspace_bytes": 2 * ws - 1}),
               ("grid > INT32_MAX", {"total_rows": 1, "count": 1 << 21, "n": n, "k": 64, "ldx": 64, "ldy": n, "ldb": n, "gate_bytes": HUGE, "up_bytes": HUGE,
                                     "workspace_bytes": HUGE})])


WS = ("workspace", "workspace_bytes")
ENTRIES = {}
TWINS = []                                     # (the (n, k) entry, its (k, n) twin), and (an entry, its _transposed form)


def _pair(stem_nk, stem_kn, tail, params, good, defects):
    a, b = f"mtq_packed_{stem_nk}{tail}", f"mtq_packed_{stem_kn}{tail}"
    ENTRIES[a] = ENTRIES[b] = (params, good, defects)
    TWINS.append((a, b))


_pair("linear", "matmul", "", SINGLE + ("stream",), SINGLE_GOOD, _block_like(BIG, 1 << 20))
_pair("linear", "matmul", "_wide", SINGLE + ("stream",), SINGLE_GOOD, _block_like(BIG, 1 << 20))
_pair("linear", "matmul", "_skinny", SINGLE + ("split",) + WS + ("stream",), SINGLE_GOOD, _skinny())
_pair("linear", "matmul", "_skinny_grouped", GROUPED + ("split",) + WS + ("stream",), GROUPED_GOOD, _skinny_grouped())
_pair("linear", "matmul", "_skinny_grouped_chunked", GROUPED + ("split",) + WS + ("stream",), GROUPED_GOOD, _chunked())
_pair("linear", "matmul", "_wide_grouped", GROUPED + WS + ("stream",), GROUPED_GOOD, _wide_grouped())
_pair("glu", "glu_matmul", "_wide", GLU_SINGLE + ("stream",), GLU_SINGLE_GOOD, _glu_wide())
_pair("glu", "glu_matmul", "_wide_grouped", GLU_GROUPED + WS + ("stream",), GLU_GROUPED_GOOD, _glu_wide_grouped())
_pair("glu", "glu_matmul", "_skinny", GLU_SINGLE + ("split",) + WS + ("stream",), GLU_SINGLE_GOOD, _glu_skinny())
_pair("glu", "glu_matmul", "_skinny_grouped", GLU_GROUPED + ("split",) + WS + ("stream",), GLU_GROUPED_GOOD, _glu_skinny_grouped())
PRODUCTS = tuple(ENTRIES)

# ---- the size functions: the shape rule's defects, and good calls at the library's split, one slice and several
SINGLE_SIZE_GOOD = dict(m=M, n=N, k=K, split=0)
GROUPED_SIZE_GOOD = dict(total_rows=T, count=COUNT, n=N, k=K, split=0)
GOOD_SINGLE = [("good", {}), ("good, split 1", {"split": 1}), ("good, split 2", {"split": 2}), ("good, split above the tiles", {"split": 9}),
               ("good, the library's split of a long k", {"k": 1 << 14, "m": 32})]
GOOD_GROUPED = [("good", {}), ("good, split 1", {"split": 1}), ("good, split 2", {"split": 2}), ("good, split above the tiles", {"split": 9}),
                ("good, the library's split of a long k", {"k": 1 << 14, "total_rows": 77, "count": 5})]
SIZES = {}
for stem_nk, stem_kn in (("linear", "matmul"), ("glu", "glu_matmul")):
    glu = stem_nk == "glu"
    for tail, params, good, defects, goods in (
            ("_skinny", ("m", "n", "k", "split"), SINGLE_SIZE_GOOD, _skinny_shape(), GOOD_SINGLE),
            ("_skinny_grouped", ("total_rows", "count", "n", "k", "split"), GROUPED_SIZE_GOOD, _grouped_shape(glu), GOOD_GROUPED),
            ("_skinny_grouped_chunked", ("total_rows", "count", "n", "k", "split"), GROUPED_SIZE_GOOD, _grouped_shape(), GOOD_GROUPED),
            ("_wide_grouped", ("total_rows", "count", "n", "k"), GROUPED_SIZE_GOOD, _no_split(_grouped_shape()), _no_split(GOOD_GROUPED))):
        if glu and tail == "_skinny_grouped_chunked":
            continue
        a, b = f"mtq_packed_{stem_nk}{tail}_workspace_bytes", f"mtq_packed_{stem_kn}{tail}_workspace_bytes"
        SIZES[a] = SIZES[b] = (params, good, defects, goods)
        TWINS.append((a, b))

# ---- pack / unpack: rows x cols = 40 x 70 is 2 x 3 tiles either way round
ROWS, COLS = 40, 70
for batched in (False, True):
    count = COUNT if batched else 1
    shape = [("count = 0", {"count": 0}), ("count < 0", {"count": -1})] if batched else []
    shape += _grid("rows", "cols")
    if batched:
        shape += [("tiles > batch max", {"rows": 1 << 20, "cols": 1 << 18}), ("tiles in the batch", {"rows": 1 << 15, "cols": 1 << 15, "count": (1 << 20) + 1})]
    for pack in (True, False):
        ld, buf, nbytes, dtype = ("ld", "out", "out_bytes", "in_dtype") if pack else ("ldy", "packed", "packed_bytes", "out_dtype")
        mat = "x" if pack else "y"
        tables = ("maps", "offsets", "bases") if batched else ("map", "offsets")
        if pack:
            params = (mat, dtype) + (("count",) if batched else ()) + ("rows", "cols", ld) + (("stride",) if batched else ()) + tables + (buf, nbytes, "stream")
        else:
            params = (buf, nbytes) + tables + (("count",) if batched else ()) + ("rows", "cols", mat, dtype, ld) + (("stride",) if batched else ()) + ("stream",)
        good = {mat: ptr(0), dtype: F32, "count": count, "rows": ROWS, "cols": COLS, ld: COLS, "stride": ROWS * COLS, "map": ptr(2), "maps": ptr(2),
                "offsets": ptr(3), "bases": ptr(9), buf: ptr(1), nbytes: count * TILES * BLOB, "stream": None}
        defects = (_nulls([p for p in params if p in (mat, buf) + tables]) + [(dtype, {dtype: 7})] + shape + [(f"{ld} < cols", {ld: COLS - 1})]
                   + ([("stride", {"stride": ROWS * COLS - 1})] if batched else [])
                   + [(f"{buf} misaligned", {buf: ptr(1) + 8}), (f"{nbytes} short", {nbytes: count * TILES * BLOB - 1})])
        a = f"mtq_{'pack' if pack else 'unpack'}_tiles{'_batched' if batched else ''}"
        b = f"mtq_{'pack' if pack else 'unpack'}_tiles_transposed{'_batched' if batched else ''}"
        ENTRIES[a] = ENTRIES[b] = (params, good, defects)
        TWINS.append((a, b))


def _rungs(defects):
    """(label, overrides) of every single defect and, behind it, of its pair with the next; the earlier defect's values win"""
    for i, (label, over) in enumerate(defects):
        yield label, over
        if i + 1 < len(defects):
            nxt_label, nxt = defects[i + 1]
            yield f"{label} + {nxt_label}", {**nxt, **over}


def ladder(name):
    """[label, return code, text] of every rung of a product or pack / unpack entry; [label, value] of a size function's"""
    L = hb.lib()
    fn = getattr(L, name)
    if name in SIZES:
        params, good, defects, goods = SIZES[name]
        out = [[label, int(fn(*[{**good, **over}[p] for p in params]))] for label, over in _rungs(defects)]
        return out + [[label, int(fn(*[{**good, **over}[p] for p in params]))] for label, over in goods]
    params, good, defects = ENTRIES[name]
    out = []
    for label, over in _rungs(defects):
        assert over, name
        rc = fn(*[{**good, **over}[p] for p in params])
        out.append([label, int(rc), L.mtq_last_error().decode()])
    return out


def all_ladders():
    return {name: ladder(name) for name in list(ENTRIES) + list(SIZES)}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        rows = [f"{json.dumps(name)}: {json.dumps(rungs, separators=(',', ':'))}" for name, rungs in sorted(all_ladders().items())]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
