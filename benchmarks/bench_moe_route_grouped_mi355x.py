#!/usr/bin/env python3
"""The grouped router (moe_topk_grouped, moe_route_grouped) against the torch composition it replaces, and against moe_topk_softmax as the cost floor of the
skeleton the two share.

  topkg   ours_us   one launch: moe_topk_grouped(logits, topk, n_group, topk_group, bias, scoring, renormalize, routed_scaling_factor)
          torch_us  the composition written out in torch_grouped below: sigmoid / softmax, add, view, topk (x2 with a bias) / max, sum, topk, scatter_, masked_fill,
                    topk, gather, sum, div, mul
          floor_us  moe_topk_softmax(logits, topk) at the same (T, E, topk): what the shared skeleton costs without scores, bias and groups
  routeg  ours_us   moe_route_grouped(...): the op above followed by moe_sort_fused
          torch_us  the torch composition followed by moe_sort
          floor_us  moe_route(logits, topk)

Every point is taken twice: `graph` -- medians of HIP-graph replays (bench_configs.time_us: device time, no host work between the launches) -- and `eager` -- a host
clock around back-to-back calls ending in a synchronise.  `spread`, `torch_spread` and `floor_spread` are (max - min) / median of each side over --repeat whole
measurements; the three sides alternate inside every repeat, so both comparisons come from the same run.  A gain counts only where it exceeds both spreads.

Shapes: DeepSeek-V3 (E 256, 8 groups, top-4 groups, top-8, bias, x 2.5), Kimi-K2 (E 384, one group, top-8, bias, x 2.827), DeepSeek-V2-Lite (E 64, one group, top-6,
softmax), DeepSeek-V2 (E 160, 8 groups, top-3 groups, top-6, softmax), each at T in {1, 64, 512, 4096}, bf16 logits.

Every (model, phase) is one GPU step: a child process of its own under its own time limit (--step-timeout), and the first step that fails or runs out of time ends the
run -- nothing more is started on a device that has just misbehaved.

    python benchmarks/bench_moe_route_grouped_mi355x.py [--repeat 3] [--quick] [--step-timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (model, E, n_group, topk_group, top-k, scoring, bias, renormalize, routed_scaling_factor)
MODELS = [("DeepSeek-V3", 256, 8, 4, 8, "sigmoid", True, True, 2.5), ("Kimi-K2", 384, 1, 1, 8, "sigmoid", True, True, 2.827),
          ("DeepSeek-V2-Lite", 64, 1, 1, 6, "softmax", False, False, 1.0), ("DeepSeek-V2", 160, 8, 3, 6, "softmax", False, False, 16.0)]
TOKENS = {"decode": [1, 64], "prefill": [512, 4096]}
STEPS = [(m, p) for m in range(len(MODELS)) for p in TOKENS]


def time_eager_us(fn, iters):
    import torch

    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def torch_grouped(logits, topk, n_group, topk_group, bias, scoring, renormalize, scale):
    """the router as model code writes it (vLLM's grouped_topk: the masked groups' experts are filled with -inf)"""
    import torch

    T, E = logits.shape
    s = logits.float().sigmoid() if scoring == "sigmoid" else torch.softmax(logits.float(), dim=-1)
    c = s + bias if bias is not None else s
    if n_group > 1:
        cg = c.view(T, n_group, E // n_group)
        gscore = cg.topk(2, dim=-1).values.sum(dim=-1) if bias is not None else cg.max(dim=-1).values
        gidx = gscore.topk(topk_group, dim=-1, sorted=False).indices
        gmask = torch.zeros_like(gscore)
        gmask.scatter_(1, gidx, 1)
        mask = gmask.unsqueeze(-1).expand(T, n_group, E // n_group).reshape(T, E)
        c = c.masked_fill(~mask.bool(), float("-inf"))
    ids = c.topk(topk, dim=-1, sorted=True).indices
    w = s.gather(1, ids)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return w * scale, ids


def run_step(model_i, phase, args):
    import numpy as np
    import torch

    from bench_configs import time_us
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    model, E, G, tg, topk, scoring, with_bias, renorm, scale = MODELS[model_i]
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}", flush=True)

    def measure(fns):
        res = {}
        for mode in ("graph", "eager"):
            t = (lambda f: time_us(f, args.iters)) if mode == "graph" else (lambda f: time_eager_us(f, args.iters))
            ts = [[] for _ in fns]
            for _ in range(max(1, args.repeat)):
                for lst, f in zip(ts, fns):
                    lst.append(t(f))
            med = [float(np.median(x)) for x in ts]
            res[mode] = [(m, (max(x) - min(x)) / m) for m, x in zip(med, ts)]
        return res

    def report(op, T, res):
        for mode, ((a_, sa), (b_, sb), (c_, sc)) in res.items():
            print(f"{op:6s} {model:16s} {phase:8s} T={T:5d} E={E:4d} G={G} topk={topk} {mode:>5s} ours_us {a_:8.2f} torch_us {b_:8.2f} floor_us {c_:8.2f} torch/ours {b_ / a_:6.2f} "
                  f"ours/floor {a_ / c_:5.2f} spread {sa:5.3f} torch_spread {sb:5.3f} floor_spread {sc:5.3f}", flush=True)
            print("JSON " + json.dumps(dict(op=op, model=model, phase=phase, T=T, E=E, n_group=G, topk_group=tg, topk=topk, scoring=scoring, bias=with_bias, mode=mode,
                                            ours_us=round(a_, 3), torch_us=round(b_, 3), floor_us=round(c_, 3), spread=round(sa, 4), torch_spread=round(sb, 4),
                                            floor_spread=round(sc, 4))), flush=True)

    for T in TOKENS[phase]:
        if args.quick and T not in (64, 4096):
            continue
        gen = torch.Generator(device="cpu").manual_seed(T)
        logits = (torch.randn(T, E, generator=gen) * 3.0).to(torch.bfloat16).to(dev)
        bias = (torch.randn(E, generator=gen) * 0.1).to(dev) if with_bias else None
        kw = dict(n_group=G, topk_group=tg, bias=bias, scoring=scoring, renormalize=renorm, routed_scaling_factor=scale)
        # the two sides compute the same routing wherever the composition has no tie to break and exp / sigmoid merge nothing: a sanity check, not a test
        w, ids = q.moe_topk_grouped(logits, topk, **kw)
        tw, tids = torch_grouped(logits, topk, G, tg, bias, scoring, renorm, scale)
        same = float((ids.long() == tids).all(dim=1).float().mean())
        print(f"# {model} T={T}: rows with the torch composition's ids {same:.4f}", flush=True)
        report("topkg", T, measure([lambda: q.moe_topk_grouped(logits, topk, **kw), lambda: torch_grouped(logits, topk, G, tg, bias, scoring, renorm, scale),
                                    lambda: q.moe_topk_softmax(logits, topk)]))
        report("routeg", T, measure([lambda: q.moe_route_grouped(logits, topk, **kw),
                                     lambda: q.moe_sort(torch_grouped(logits, topk, G, tg, bias, scoring, renorm, scale)[1], E), lambda: q.moe_route(logits, topk)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (the three sides alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="T = 64 and 4096 only")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one (model, phase) step may take")
    ap.add_argument("--step", type=int, default=-1, help=argparse.SUPPRESS)   # (internal: run this one step in this process)
    args = ap.parse_args()
    if args.step >= 0:
        run_step(*STEPS[args.step], args)
        return 0
    for i, (m, phase) in enumerate(STEPS):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(i), "--repeat", str(args.repeat), "--iters", str(args.iters)] + (["--quick"] if args.quick else [])
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"step {MODELS[m][0]} {phase}: no result within {args.step_timeout} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"step {MODELS[m][0]} {phase}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
