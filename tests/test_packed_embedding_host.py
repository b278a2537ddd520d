"""CPU-only: include/mtq_packed_gather.h against PACKED_GATHER_SIGNATURES, what mtq_packed_embedding refuses without a device, the
emulation route of packed.embedding against the whole unpacked table, and PackedEmbedding's shapes and head()."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from quantization_analysis_amd import hip_backend as hb, packed
from tests.inputs import gen
from tests.packed_cases import random_map

LETTER = {"int": "i", "int64_t": "l", "size_t": "z", "double": "d"}
SHAPES = ((70, 72), (33, 8), (96, 2080), (64, 4128))


def test_header_is_the_signature_table_and_the_names_are_optional():
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).parents[1] / "include" / "mtq_packed_gather.h").read_text(), flags=re.S)
    found = {}
    for result, name, params in re.findall(r"^(int|size_t) (mtq_\w+)\(([^;]*)\);", text, flags=re.M):
        kinds = ["p" if "*" in p else LETTER[p.split()[0]] for p in params.replace("\n", " ").split(",")]
        found[name] = (LETTER[result], "".join(kinds), True)
    assert found == hb.PACKED_GATHER_SIGNATURES and hb.PACKED_GATHER_EXPORTS == tuple(found) and hb.packed_gather_available()
    assert not set(found) & set(hb.EXPORTS) and hb.lib().mtq_version() == 143


def test_c_abi_refusals_without_a_device():
    L = hb.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16          # a 16-byte aligned host address: no check may dereference it
    # ids, id_dtype, tokens, id_first, packed, packed_bytes, map, offsets, rows, cols, stored, has_scale, scale, y, out_dtype, ldy, stream
    ok = (p, 1, 5, 0, p, 1 << 20, p, p, 70, 72, 0, 0, 0.0, p, 0, 72, None)

    def call(**kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.mtq_packed_embedding(*args), L.mtq_last_error()

    cases = [({f"a{null}": None}, b"null argument") for null in (0, 4, 6, 7, 13)]
    cases += [({"a1": 2}, b"id_dtype"), ({"a14": 5}, b"out_dtype"), ({"a10": 2}, b"stored"), ({"a2": 0}, b"tokens"), ({"a8": 0}, b"rows and cols"),
              ({"a9": -1}, b"rows and cols"), ({"a15": 71}, b"ldy"), ({"a10": 1, "a15": 69}, b"ldy"),
              ({"a4": p + 8}, b"16-byte aligned"), ({"a5": 9 * 320 - 1}, b"packed_bytes"), ({"a0": p + 4}, b"ids is not aligned"),
              ({"a13": p + 1}, b"y is not aligned")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    if not torch.cuda.is_available():     # everything in order: only the device is missing; a transposed stream's hidden size is rows = 70
        assert call()[0] == -3 and call(a1=0, a0=p + 4, a11=1, a12=8.5, a14=1)[0] == -3 and call(a5=9 * 320)[0] == -3
        assert call(a10=1, a15=71)[0] == -3


@pytest.mark.parametrize("stored", packed.MOE_STORED)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_emulation_is_the_unpacked_tables_rows(shape, stored):
    vocab, hidden = shape
    w = gen("heavy_f32", vocab + hidden, shape)
    if stored == "transpose":
        pt = packed.pack_transposed(w, random_map((hidden, vocab), 7))
        table = packed.unpack_transposed(pt)
    else:
        pt = packed.pack(w, random_map(shape, 7))
        table = packed.unpack(pt)
    ids = np.array([[0, 31, 32, vocab - 1, 5], [5, -1, vocab, 2 ** 40, 33 % vocab]])
    for id_first in (0, 32):
        at = ids - id_first
        inside = (at >= 0) & (at < vocab)
        want = np.where(inside[..., None], table[np.where(inside, at, 0)], np.float32(0))
        got = packed.embedding(ids, pt, out_dtype="float32", stored=stored, id_first=id_first)
        assert got.shape == (2, 5, hidden) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        half = packed.embedding(torch.from_numpy(ids), pt, stored=stored, id_first=id_first)
        assert half.dtype == torch.bfloat16 and np.array_equal(half.float().numpy(), want)
        scale = np.float32(np.sqrt(hidden))
        scaled = packed.embedding(ids, pt, out_dtype="float32", stored=stored, id_first=id_first, scale=scale)
        assert np.array_equal(scaled, (want.astype(np.float64) * np.float64(scale)).astype(np.float32))


def test_the_module_keeps_the_ids_shape_and_its_head_shares_the_tensor():
    w = gen("heavy_f32", 1, (70, 72))
    rows, cols = packed.pack(w, random_map((70, 72), 2)), packed.pack_transposed(w, random_map((72, 70), 3))
    for pt, stored, head in ((rows, "rows", packed.PackedLinear), (cols, "transpose", packed.PackedMatmul)):
        emb = packed.PackedEmbedding(pt, stored=stored, out_dtype="float32")
        assert (emb.num_embeddings, emb.embedding_dim) == (70, 72)
        for lead in ((), (4,), (3, 5), (2, 0, 3)):
            ids = torch.randint(0, 70, lead, generator=torch.Generator().manual_seed(1))
            y = emb(ids)
            assert tuple(y.shape) == lead + (72,) and y.dtype == torch.float32
            assert np.array_equal(y.numpy(), packed.embedding(ids, pt, out_dtype="float32", stored=stored))
        h = emb.head(out_dtype="bfloat16")
        assert type(h) is head and h.packed is pt and (h.in_features, h.out_features) == (72, 70)
    with pytest.raises(hb.MtqError, match="stored must be"):
        packed.PackedEmbedding(rows, stored="columns")
