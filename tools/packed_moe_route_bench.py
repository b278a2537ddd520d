"""The MoE router (mtq_moe_route, packed.moe_route, PackedMoE.forward_logits) against the torch sequence it replaces, by the method of
DESIGN.md §A.6g: device events after a warm-up, the sides alternated in one process, --rounds rounds of a window each, medians and
minima, the C entry called directly with prebuilt arguments.

  route   ours   : mtq_moe_route, one launch from the logits to (topk_ids, topk_weights);
          torch  : torch_route below, the sequence the models' own code runs: softmax or sigmoid, + bias, a view as groups, top-2 per
                   group and their sum (or the maximum), top-k groups, a scatter mask and masked_fill, top-k experts, a gather of the
                   unbiased scores, their sum, a divide, a scale;
  layer   ours   : PackedMoE.forward_logits;      torch: torch_route, then the same module's forward.

Routings: the four presets of packed.MOE_ROUTINGS at their models' expert counts (mixtral 8, qwen3-moe 128, deepseek-v2 160,
deepseek-v3 256, the last with a bias), float32 logits, T in --tokens.  Before any timing the ids are compared with torch's on the
tokens where they can be expected to agree (torch.topk's order among equal keys is unspecified) and the weights by their largest
difference.  The layer rows use a reduced layer (k = n = --layer-k, hidden --layer-hidden, all-bfp8 experts): they show the router's
share of a forward, not a model's speed.

The accuracy figures: the emitted scores of the kernel, and torch's float32 softmax / sigmoid on the same device, both against
torch's float64 on the generator of the tests (each row a permutation of (e - count // 2) * 8 / max(count, 8)), as the largest
relative error, beside the tests' bound (2 * ceil(8 log2 e) + ceil(log2 count) + 8) * 2^-24.

  python tools/packed_moe_route_bench.py [--rounds 3] [--window-ms 20] [--out profiles/packed_moe_route.txt] [--json out.json] [--no-layer]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd import packed
from tools.packed_glu_bench import time_sides
from tools.packed_moe_bench import experts_of

COUNTS = {"mixtral": 8, "qwen3-moe": 128, "deepseek-v2": 160, "deepseek-v3": 256}


def torch_route(logits, r: packed.MoERouting, bias):
    """(topk_weights, topk_ids) as the models' own routers compute them."""
    T, count = logits.shape
    s = torch.softmax(logits, dim=-1, dtype=torch.float32) if r.score == "softmax" else logits.float().sigmoid()
    key = s if bias is None else s + bias
    if r.n_group > 1:
        groups = key.view(T, r.n_group, -1)
        group_scores = groups.topk(2, dim=-1)[0].sum(dim=-1) if r.group_top == 2 else groups.max(dim=-1).values
        kept = group_scores.topk(r.topk_group, dim=-1, sorted=False)[1]
        group_mask = torch.zeros_like(group_scores).scatter_(1, kept, 1)
        mask = group_mask.unsqueeze(-1).expand(T, r.n_group, count // r.n_group).reshape(T, -1)
        key = key.masked_fill(~mask.bool(), float("-inf"))
    ids = key.topk(r.topk, dim=-1)[1]
    w = s.gather(1, ids)
    if r.renormalize:
        w = w / (w.sum(dim=-1, keepdim=True) + r.eps)
    return w * r.scale, ids


def generator_logits(tokens: int, count: int, seed: int):
    rng = np.random.default_rng(seed)
    base = ((np.arange(count) - count // 2) * (8.0 / max(count, 8))).astype(np.float32)
    return torch.from_numpy(np.stack([base[rng.permutation(count)] for _ in range(tokens)])).cuda()


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--routings", default="mixtral,qwen3-moe,deepseek-v2,deepseek-v3")
    p.add_argument("--tokens", default="1,16,128,512,4096")
    p.add_argument("--layer-routings", default="mixtral,deepseek-v3")
    p.add_argument("--layer-tokens", default="1,16,512")
    p.add_argument("--layer-k", type=int, default=2048)
    p.add_argument("--layer-hidden", type=int, default=512)
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--no-layer", action="store_true", help="skip the end-to-end rows (they pack the experts of a layer)")
    p.add_argument("--out", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if args.rounds < 3:
        p.error("--rounds must be at least 3")
    torch.cuda.set_device(0)
    hb.require_gpu()
    stream = torch.cuda.current_stream().cuda_stream
    route_fn = hb._entry("mtq_moe_route")
    rows_out, lines = [], []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(label, sides):
        ours, theirs = (statistics.median(s["ts"]) for s in sides)
        for s in sides:
            med, mn = statistics.median(s["ts"]), min(s["ts"])
            rows_out.append({**label, "side": s["name"], "us_median": med * 1e3, "us_min": mn * 1e3})
            say(f"{s['name']:6s} {med * 1e3:9.1f} us (min {mn * 1e3:9.1f}, spread {(med - mn) / med * 100:4.1f}%)")
        ratio = theirs / ours
        rows_out.append({**label, "side": "torch/ours", "ratio": ratio})
        say(f"torch / ours {ratio:6.2f}x" if ratio >= 1 else f"**torch / ours {ratio:6.2f}x: the kernel loses**")

    say(f"# MoE router on {torch.cuda.get_device_name(0)}; device events, {args.rounds} rounds of ~{args.window_ms:.0f} ms windows, sides "
        f"alternated; float32 logits; seed {args.seed}")
    say("## scores against float64 (largest relative error on the tests' generator, 64 tokens)")
    for count in (8, 128, 160, 256, 384, 4096):
        x = generator_logits(64, count, args.seed + count)
        bound = (2 * math.ceil(8 * math.log2(math.e)) + math.ceil(math.log2(count)) + 8) * 2.0 ** -24
        for score in ("softmax", "sigmoid"):
            want = torch.softmax(x.double(), dim=-1) if score == "softmax" else x.double().sigmoid()
            ours = packed.moe_route(x, 1, score, return_scores=True)[2].double()
            theirs = (torch.softmax(x, dim=-1) if score == "softmax" else x.sigmoid()).double()
            e_ours, e_torch = (float(((v - want).abs() / want).max()) for v in (ours, theirs))
            rows_out.append({"what": "scores", "count": count, "score": score, "kernel": e_ours, "torch_float32": e_torch, "bound": bound})
            say(f"count {count:5d} {score:8s} kernel {e_ours:.3e}  torch float32 {e_torch:.3e}  bound {bound:.3e}")
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    for name in (m for m in args.routings.split(",") if m):
        r, count = packed.MOE_ROUTINGS[name], COUNTS[name]
        bias = torch.rand((count,), generator=g, device="cuda") * 0.25 if r.expects_bias else None
        for T in (int(v) for v in args.tokens.split(",")):
            logits = torch.randn((T, count), generator=g, device="cuda")
            w, ids, s = packed.moe_route(logits, r.topk, r.score, bias, r.n_group, r.topk_group, r.group_top, r.renormalize, r.eps, r.scale,
                                         return_scores=True)
            w_t, ids_t = torch_route(logits, r, bias)
            same = (ids.long() == ids_t).all(dim=-1)
            diff = float((w[same] - w_t[same]).abs().max()) if bool(same.any()) else float("nan")
            say(f"## {name}: count={count} K={r.topk} groups={r.n_group}/{r.topk_group} T={T}: ids equal to torch's on "
                f"{int(same.sum())} of {T} tokens; weights max abs diff there {diff:.3e}")
            ids_o, w_o = torch.empty_like(ids), torch.empty_like(w)
            call = (logits.data_ptr(), hb.DTYPE_F32, count, T, count, r.topk, hb.ROUTE_SCORES[r.score], None if bias is None else bias.data_ptr(),
                    r.n_group, r.topk_group, r.group_top, int(r.renormalize), float(r.eps), float(r.scale), ids_o.data_ptr(), r.topk,
                    w_o.data_ptr(), r.topk, None, 0, stream)
            sides = [{"name": "ours", "fn": lambda i: hb.check(route_fn(*call))}, {"name": "torch", "fn": lambda i: torch_route(logits, r, bias)}]
            time_sides(sides, args.rounds, args.window_ms)
            report({"what": "route", "routing": name, "count": count, "K": r.topk, "T": T}, sides)
    if not args.no_layer:
        k, hidden = args.layer_k, args.layer_hidden
        for name in (m for m in args.layer_routings.split(",") if m):
            r, count = packed.MOE_ROUTINGS[name], COUNTS[name]
            moe = packed.PackedMoE(*experts_of(count, k, hidden, args.seed), decode_max_rows=256, router=name)
            bias = torch.rand((count,), generator=g, device="cuda") * 0.25 if r.expects_bias else None
            for T in (int(v) for v in args.layer_tokens.split(",")):
                logits = torch.randn((T, count), generator=g, device="cuda")
                x = torch.randn((T, k), generator=g, device="cuda").to(torch.bfloat16)

                def layer_torch(i):
                    w_t, ids_t = torch_route(logits, r, bias)
                    return moe(x, ids_t, w_t)

                a, b = moe.forward_logits(x, logits, bias=bias), layer_torch(0)
                say(f"## layer {name}: count={count} K={r.topk} k=n={k} hidden={hidden} T={T}: max abs diff to torch routing + forward "
                    f"{float((a.float() - b.float()).abs().max()):.3e}")
                sides = [{"name": "ours", "fn": lambda i: moe.forward_logits(x, logits, bias=bias)}, {"name": "torch", "fn": layer_torch}]
                time_sides(sides, args.rounds, args.window_ms)
                report({"what": "layer", "routing": name, "count": count, "K": r.topk, "k": k, "hidden": hidden, "T": T}, sides)
            del moe
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if args.json:
        Path(args.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
