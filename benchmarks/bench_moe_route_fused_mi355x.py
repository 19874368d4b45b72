#!/usr/bin/env python3
"""One-launch MoE routing for decode against the two launches it replaces, and the bound up to which the torch ops take it.

  fused_us  the C entry qutlass_amd_moe_route_fused / qutlass_amd_moe_route_grouped_fused on preallocated results: ALWAYS one launch of one workgroup
  two_us    moe_route / moe_route_grouped of the same build: the router's launch, then moe_sort_fused's (and the fill that zeroes offs)
  op_us     the shipped op, moe_route_fused / moe_route_grouped_fused (torch.ops.qutlass_amd.*): it allocates its five results, takes the one launch up to
            qutlass_amd_moe_route_fused_max_tokens() tokens and the two bare entries beyond, and launches no fill in either case -- up to the bound it is fused_us
            plus nothing on the device, beyond it twoc_us
  twoc_us   the same two launches as bare C entries (qutlass_amd_moe_topk_* then qutlass_amd_moe_sort) on preallocated results -- what the ops
            qutlass_amd::moe_route_fused / moe_route_grouped_fused run beyond the bound; for information, the bound rule does not read it

All four as replayed HIP graphs (bench_configs.time_us: device time, no host work between the launches): medians of --repeat measurements of --iters calls, the
sides alternating inside every repeat; `*_spread` is (max - min) / median of a side over the repeats.  Before anything is timed the four sides' five results are
compared: they are equal bit for bit.

The bound B (qutlass_amd_moe_route_fused_max_tokens): the largest T of the sweep such that at it and at every smaller T of the sweep fused_us is below two_us for
EVERY router, by more than max - min of either side at that cell.  0 if there is no such T.  The rule that fixed MOE_SORT_ONE_LAUNCH_MAX.  The last line also gives
the same rule with op_us in the place of fused_us: how far the shipped op, which switches forms at the bound, beats moe_route.

Routers: Mixtral-8x7B (E 8, top-2), gpt-oss-120b (E 128, top-4), Qwen3-30B-A3B (E 128, top-8), DeepSeek-V3 (E 256, 8 groups, top-4 groups, top-8, bias, x 2.5),
Kimi-K2 (E 384, one group, top-8, bias, x 2.827), at T in {1, 2, 4, 8, 16, 32, 64}, bf16 logits.

Every router is one GPU step: a child process of its own under its own time limit (--step-timeout), and the first step that fails or runs out of time ends the run --
nothing more is started on a device that has just misbehaved.

    python benchmarks/bench_moe_route_fused_mi355x.py [--repeat 3] [--iters 100] [--step-timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (model, E, top-k, grouped router or None: (n_group, topk_group, scoring, bias, routed_scaling_factor))
MODELS = [("Mixtral-8x7B", 8, 2, None), ("gpt-oss-120b", 128, 4, None), ("Qwen3-30B-A3B", 128, 8, None),
          ("DeepSeek-V3", 256, 8, (8, 4, "sigmoid", True, 2.5)), ("Kimi-K2", 384, 8, (1, 1, "sigmoid", True, 2.827))]
TOKENS = [1, 2, 4, 8, 16, 32, 64]


def run_step(model_i, args):
    import numpy as np
    import torch

    from bench_configs import time_us
    import qutlass_amd as q

    lib = q._lib.load()
    dev = torch.device("cuda:0")
    model, E, topk, grouped = MODELS[model_i]
    print(f"# {lib.qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}", flush=True)
    bias = None
    if grouped:
        n_group, topk_group, scoring, has_bias, scale = grouped
        if has_bias:
            bias = (torch.randn(E, generator=torch.Generator(device="cpu").manual_seed(E)) * 0.1).to(dev)
    for T in TOKENS:
        logits = (torch.randn(T, E, generator=torch.Generator(device="cpu").manual_seed(T)) * 3.0).to(torch.bfloat16).to(dev)

        def outputs():
            i32 = dict(dtype=torch.int32, device=dev)
            return [torch.empty(T, topk, dtype=torch.float32, device=dev), torch.empty(T, topk, **i32), torch.empty(T * topk, **i32), torch.zeros(E, **i32),
                    torch.empty(T, topk, **i32)]

        of, oc = outputs(), outputs()
        pf, pc = [o.data_ptr() for o in of], [o.data_ptr() for o in oc]
        bp = bias.data_ptr() if bias is not None else None

        def stream():
            return torch.cuda.current_stream().cuda_stream

        if grouped:
            code = q._lib.MOE_SCORING[scoring]

            def fused():
                q._lib.check(lib.qutlass_amd_moe_route_grouped_fused(logits.data_ptr(), 2, T, E, topk, n_group, topk_group, code, bp, 1, scale, pf[0], pf[1], E, None, 0,
                                                                     pf[2], pf[3], pf[4], stream()))

            def two():
                return q.moe_route_grouped(logits, topk, n_group=n_group, topk_group=topk_group, bias=bias, scoring=scoring, routed_scaling_factor=scale)

            def op():
                return q.moe_route_grouped_fused(logits, topk, n_group=n_group, topk_group=topk_group, bias=bias, scoring=scoring, routed_scaling_factor=scale)

            def twoc():
                q._lib.check(lib.qutlass_amd_moe_topk_grouped(logits.data_ptr(), 2, T, E, topk, n_group, topk_group, code, bp, 1, scale, pc[0], pc[1], None, stream()))
                q._lib.check(lib.qutlass_amd_moe_sort(pc[1], 4, T, topk, E, None, 0, pc[2], pc[3], pc[4], None, 0, stream()))
        else:
            def fused():
                q._lib.check(lib.qutlass_amd_moe_route_fused(logits.data_ptr(), 2, T, E, topk, 1, pf[0], pf[1], E, None, 0, pf[2], pf[3], pf[4], stream()))

            def two():
                return q.moe_route(logits, topk)

            def op():
                return q.moe_route_fused(logits, topk)

            def twoc():
                q._lib.check(lib.qutlass_amd_moe_topk_softmax(logits.data_ptr(), 2, T, E, topk, 1, pc[0], pc[1], stream()))
                q._lib.check(lib.qutlass_amd_moe_sort(pc[1], 4, T, topk, E, None, 0, pc[2], pc[3], pc[4], None, 0, stream()))

        fused()
        twoc()
        ref, shipped = two(), op()
        torch.cuda.synchronize()
        for side, got in (("fused", of), ("twoc", oc), ("op", shipped)):
            for name, a, b in zip(("weights", "ids", "src_row", "offs", "pos"), got, ref):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{model} T={T}: {side} {name} differs from moe_route's"
        sides = {"fused": fused, "op": op, "two": two, "twoc": twoc}
        ts = {k: [] for k in sides}
        for _ in range(max(1, args.repeat)):
            for k, fn in sides.items():
                ts[k].append(time_us(fn, args.iters))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rng = {k: max(v) - min(v) for k, v in ts.items()}
        gain = med["two"] - med["fused"]
        wins = gain > max(rng["fused"], rng["two"])
        wins_op = med["two"] - med["op"] > max(rng["op"], rng["two"])
        print(f"route_fused {model:14s} T={T:3d} E={E:4d} topk={topk} graph fused_us {med['fused']:7.2f} op_us {med['op']:7.2f} two_us {med['two']:7.2f} twoc_us {med['twoc']:7.2f} "
              f"two/fused {med['two'] / med['fused']:5.2f} two/op {med['two'] / med['op']:5.2f} twoc/fused {med['twoc'] / med['fused']:5.2f} "
              f"fused_spread {rng['fused'] / med['fused']:5.3f} op_spread {rng['op'] / med['op']:5.3f} two_spread {rng['two'] / med['two']:5.3f} twoc_spread {rng['twoc'] / med['twoc']:5.3f} {'WINS' if wins else 'no win'}", flush=True)
        print("JSON " + json.dumps(dict(op="route_fused", model=model, T=T, E=E, topk=topk, fused_us=round(med["fused"], 3), op_us=round(med["op"], 3), op_range_us=round(rng["op"], 3), two_us=round(med["two"], 3),
                                        twoc_us=round(med["twoc"], 3), fused_range_us=round(rng["fused"], 3), two_range_us=round(rng["two"], 3),
                                        twoc_range_us=round(rng["twoc"], 3), wins=bool(wins), wins_op=bool(wins_op))), flush=True)


def bound(rows, key="wins"):
    """the rule of the module docstring over the JSON rows of a complete sweep (key "wins_op": the same rule with op_us in the place of fused_us)"""
    b = 0
    for T in TOKENS:
        cells = [r for r in rows if r["T"] == T]
        if len(cells) != len(MODELS) or not all(r[key] for r in cells):
            break
        b = T
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per cell (the sides alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one router's step may take")
    ap.add_argument("--step", type=int, default=-1, help=argparse.SUPPRESS)   # (internal: run this one step in this process)
    args = ap.parse_args()
    if args.step >= 0:
        run_step(args.step, args)
        return 0
    rows = []
    for i, (model, *_) in enumerate(MODELS):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(i), "--repeat", str(args.repeat), "--iters", str(args.iters)]
        try:
            done = subprocess.run(cmd, timeout=args.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"step {model}: no result within {args.step_timeout} s; stopping", flush=True)
            return 124
        print(done.stdout, end="", flush=True)
        if done.returncode != 0:
            print(f"step {model}: exit status {done.returncode}; stopping", flush=True)
            return done.returncode
        rows += [json.loads(line[5:]) for line in done.stdout.splitlines() if line.startswith("JSON ")]
    import qutlass_amd as q

    print(f"bound: the one launch wins for every router, beyond both sides' max - min, at every T of the sweep up to B = {bound(rows)} "
          f"(this build's qutlass_amd_moe_route_fused_max_tokens() = {q._lib.load().qutlass_amd_moe_route_fused_max_tokens()}); the shipped op beats moe_route / "
          f"moe_route_grouped by the same rule at every T of the sweep up to {bound(rows, 'wins_op')}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
