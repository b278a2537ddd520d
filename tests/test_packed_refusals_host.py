"""CPU-only: what the packed C entries of csrc/mtq_packed.hip refuse, in which order and in which words.  Every rung of every ladder of
tests/packed_refusal_cases.py is held to tests/golden/packed_refusals.json, text for text; the fixture was recorded by running that module
as a script against the library before the (n, k) and (k, n) entries came to share their host bodies.  Independently of the fixture, a
pair call reports the earlier of its two defects, and the two members of a twin pair answer every rung alike.  No call reaches a
device."""
import json
import re
from pathlib import Path

import pytest

from tests import packed_refusal_cases as cases

GOLDEN = json.loads((Path(__file__).parent / "golden" / "packed_refusals.json").read_text())
NAMES = list(cases.ENTRIES) + list(cases.SIZES)


def _digits(text):
    """a text with its numbers blanked: the workspace texts quote sizes, which a pair's other defect may change"""
    return re.sub(r"\d+", "#", text)


def test_the_ladders_cover_every_entry_and_both_members_of_every_pair():
    assert len(cases.PRODUCTS) == 20 and len(cases.SIZES) == 14 and len(cases.ENTRIES) == 28
    assert sorted(GOLDEN) == sorted(NAMES)
    from quantization_analysis_amd import hip_backend as hb
    in_scope = [name for name in hb.SIGNATURES if name.startswith(("mtq_packed_linear", "mtq_packed_matmul", "mtq_packed_glu", "mtq_pack_tiles", "mtq_unpack_tiles"))]
    assert sorted(in_scope) == sorted(NAMES)
    assert len(cases.TWINS) == 21 and sorted(name for pair in cases.TWINS for name in pair) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_an_entry_refuses_what_it_refused_in_the_same_words_and_order(name):
    got = cases.ladder(name)
    assert [rung[0] for rung in got] == [rung[0] for rung in GOLDEN[name]]
    for rung, want in zip(got, GOLDEN[name]):
        assert rung == want, (name, rung[0])
    if name in cases.SIZES:
        refusals = [rung for rung in got if not rung[0].startswith("good")]
        assert refusals and all(value == 2 ** 64 - 1 for _label, value in refusals)
        assert all(value != 2 ** 64 - 1 for label, value in got if label.startswith("good"))
        return
    by_label = {label: (rc, text) for label, rc, text in got}
    assert all(rc != 0 and text for rc, text in by_label.values()), name
    pairs = [label for label in by_label if " + " in label]
    assert len(pairs) == len(cases.ENTRIES[name][2]) - 1
    for label in pairs:
        rc, text = by_label[label]
        first_rc, first_text = by_label[label.split(" + ")[0]]
        assert (rc, _digits(text)) == (first_rc, _digits(first_text)), (name, label)


@pytest.mark.parametrize("name,twin", cases.TWINS)
def test_a_twin_pair_answers_every_rung_alike(name, twin):
    assert cases.ladder(name) == cases.ladder(twin)
