"""Recorded layer inputs and outputs for the layer-output error (output_error.py, scripts/layer_output_error.py).

Two sources:
  * a directory in the layout of the reference's scripts/generate_deepseek_layer0_io.py:
    `<io_root>/<op path with "." → "/">/<split>/sample_NNNN.pt`, splits `calibration` and `test`, the sample index global across
    splits, each file a torch.save'd dict {"args", "kwargs", "output", "sample_idx", "split"} of one forward call of the op;
  * `synthetic:<tokens>[:seed]` — N(0, 1) bf16 activations of <tokens> rows for every 2-D weight of the model index, no recorded
    output (benchmarks, offline use with the `synthetic:deepseek-r1-layer0` preset).
An op is `<op>.weight` of the model index (plus `<op>.bias` when the index has it); ops are selected with wq's filter rules.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterator, Optional

from .model_source import ModelIndex, filter_tensor_names

SPLITS = ("calibration", "test")
_SAMPLE = re.compile(r"^sample_(\d+)\.pt$")


@dataclass
class OpIO:
    """One op's weight names and its samples.  samples: (split, sample_idx, path) in sample order; for a synthetic source the
    single entry ("synthetic", seed, None) with `tokens` rows."""

    op: str
    weight: str
    bias: Optional[str]
    samples: list = field(default_factory=list)
    tokens: int = 0

    @property
    def splits(self) -> list[str]:
        return sorted({s for s, _, _ in self.samples})


@dataclass
class Chunk:
    x: object                  # torch (m, k) bfloat16, host
    recorded: object = None    # torch (m, n) host tensor or None
    cast: bool = False         # X.to(bfloat16) changed a value


def is_synthetic(io_root: str) -> bool:
    return str(io_root).startswith("synthetic:")


def _parse_synthetic(io_root: str) -> tuple[int, int]:
    parts = str(io_root).split(":")
    try:
        tokens = int(parts[1])
        seed = int(parts[2]) if len(parts) > 2 else 0
    except (IndexError, ValueError):
        raise ValueError(f"'{io_root}': expected synthetic:<tokens>[:seed]") from None
    if tokens <= 0:
        raise ValueError(f"'{io_root}': <tokens> must be positive")
    return tokens, seed


def discover_ops(io_root) -> dict[str, list]:
    """op name → [(split, sample_idx, path)] sorted by sample index, for every directory holding a split directory of samples."""
    root = Path(io_root)
    if not root.is_dir():
        raise FileNotFoundError(f"{root}: not a directory")
    ops: dict[str, list] = {}
    for split in SPLITS:
        for split_dir in sorted(root.rglob(split)):
            if not split_dir.is_dir():
                continue
            rel = split_dir.parent.relative_to(root)
            if not rel.parts:
                continue
            files = []
            for p in split_dir.iterdir():
                mt = _SAMPLE.match(p.name)
                if mt and p.is_file():
                    files.append((split, int(mt.group(1)), p))
            if files:
                ops.setdefault(".".join(rel.parts), []).extend(files)
    for v in ops.values():
        v.sort(key=lambda t: (t[1], t[0]))
    return ops


def select_ops(index: ModelIndex, io_root, filter_query: Optional[str], split: str = "all", max_samples: Optional[int] = None):
    """→ (ops, skipped): the OpIO of every op whose weight matches `filter_query` (wq's rules on the `<op>.weight` names), and
    [(op, reason)] for ops the index cannot serve.  split: "calibration", "test" or "all"; max_samples: the first N samples of the
    selection (by global sample index)."""
    if split not in ("all",) + SPLITS:
        raise ValueError(f"split must be one of calibration, test, all; got {split!r}")
    names = set(index.tensor_names)
    skipped: list[tuple[str, str]] = []
    if is_synthetic(io_root):
        tokens, seed = _parse_synthetic(io_root)
        ops = {}
        for name in index.tensor_names:
            if not name.endswith(".weight"):
                continue
            shape, _ = index.shape_dtype(name)
            if len(shape) == 2:
                ops[name[: -len(".weight")]] = [("synthetic", seed, None)]
    else:
        ops = discover_ops(io_root)
    weights = filter_tensor_names([f"{op}.weight" for op in ops], filter_query)
    out = []
    for wname in weights:
        op = wname[: -len(".weight")]
        if wname not in names:
            skipped.append((op, f"no tensor {wname} in the model index"))
            continue
        samples = ops[op]
        if split != "all" and not is_synthetic(io_root):
            samples = [s for s in samples if s[0] == split]
        if max_samples is not None:
            samples = samples[: max(0, int(max_samples))]
        if not samples:
            skipped.append((op, f"no samples in split {split!r}"))
            continue
        bias = f"{op}.bias" if f"{op}.bias" in names else None
        out.append(OpIO(op=op, weight=wname, bias=bias, samples=samples, tokens=tokens if is_synthetic(io_root) else 0))
    return out, skipped


def _input_of(payload: dict):
    import torch

    args = payload.get("args") or ()
    if len(args) > 0 and torch.is_tensor(args[0]):
        return args[0]
    kwargs = payload.get("kwargs") or {}
    for key in ("input", "hidden_states", "x"):
        if torch.is_tensor(kwargs.get(key)):
            return kwargs[key]
    for v in kwargs.values():
        if torch.is_tensor(v):
            return v
    return None


def load_sample(path) -> dict:
    import torch

    return torch.load(str(path), map_location="cpu", weights_only=False)


def check_op(op: OpIO, w_shape: tuple) -> Optional[str]:
    """Why the op cannot be evaluated (None = it can), from the weight shape and its first sample."""
    if len(w_shape) != 2:
        return f"weight is {len(w_shape)}-D {tuple(w_shape)}, not 2-D"
    if op.tokens:
        return None
    import torch

    payload = load_sample(op.samples[0][2])
    x = _input_of(payload)
    if x is None:
        return "no tensor input in args or kwargs"
    if x.shape[-1] != w_shape[1]:
        return f"input last dim {x.shape[-1]} != weight in-features {w_shape[1]} (Conv1D-style [in, out] weights are not supported)"
    out = payload.get("output")
    if not torch.is_tensor(out):
        return f"output is a {type(out).__name__}, not a tensor"
    if out.dim() < 1 or out.shape[-1] != w_shape[0]:
        return f"output last dim {out.shape[-1] if out.dim() else None} != weight out-features {w_shape[0]}"
    return None


def chunks(op: OpIO, k: int, n: int, max_rows: int = 16384) -> Iterator[Chunk]:
    """The op's activations as (m, k) bf16 host chunks of at most max_rows rows (a sample is never split across two chunks unless it
    alone is longer), with the recorded outputs as (m, n) when the source has them."""
    import torch

    if op.tokens:
        _, seed, _ = op.samples[0]
        g = torch.Generator()
        g.manual_seed(seed)
        done = 0
        while done < op.tokens:
            m = min(max_rows, op.tokens - done)
            yield Chunk(x=torch.randn((m, k), generator=g).to(torch.bfloat16))
            done += m
        return
    for _, _, path in op.samples:
        payload = load_sample(path)
        x = _input_of(payload).reshape(-1, k)
        xb = x.to(torch.bfloat16)
        cast = x.dtype != torch.bfloat16 and not torch.equal(xb.to(x.dtype), x)
        out = payload.get("output")
        rec = out.reshape(-1, n) if torch.is_tensor(out) else None
        if rec is not None and rec.dtype not in (torch.bfloat16, torch.float32):
            rec = rec.float()
        for s in range(0, xb.shape[0], max_rows):
            yield Chunk(x=xb[s: s + max_rows], recorded=None if rec is None else rec[s: s + max_rows], cast=cast)
