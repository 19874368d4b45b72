#!/usr/bin/env python3
"""The NVFP4 MoE dispatch with one global scale per expert: what does looking the scale up per row cost, and what does it save?

  grouped_us   one launch: fusedGatherQuantizeNvGrouped(x, h, global_scales (E,), src_row, offs)
  single_us    one launch of the single-scale kernel on the same operands: fusedGatherQuantizeNv(x, h, global_scales[0:1], src_row) -- the bytes are NOT what a
               per-expert checkpoint needs; this is the floor the grouped-scale kernel is measured against
  loop_us      the only other way to honour E scales: fusedGatherQuantizeNv once per non-empty expert on its row range of src_row, with the group boundaries already
               on the host (the device-to-host copy of offs and its sync, which a real caller pays on every layer, are NOT in the figure)
  spread       (max - min) / median of the grouped time over --repeat whole measurements of the row (the three forms alternate)

Timing as benchmarks/bench_moe_dispatch_mi355x.py: medians of HIP-graph replays, WARM (one input replayed) and COLD (inputs rotated so that a cycle exceeds 1 GiB --
or 40 inputs of a small shape).  Shapes and routings are that benchmark's: Qwen3-30B-A3B (H = 2048, E = 128, top-8) and Mixtral-8x7B (H = 4096, E = 8, top-2) at
decode (64 tokens) and prefill (4096 tokens), uniform and skewed routing; R = 16 and R = 128.

Every (model, phase) is one GPU step: a child process of its own under its own time limit (--step-timeout), and the first step that fails or runs out of time ends the
run -- nothing more is started on a device that has just misbehaved.

    python benchmarks/bench_moe_grouped_scales_mi355x.py [--repeat 3] [--quick] [--step-timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_moe_dispatch_mi355x import MODELS, STEPS, TOKENS, _hadamard, topk_ids  # noqa: E402  (the dispatch benchmark's layers and routings)

ROTS = (16, 128)


def run_step(model_i, phase, args):
    import numpy as np
    import torch

    from bench_configs import time_us, time_us_cold
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    model, H, E, topk = MODELS[model_i]
    T = TOKENS[phase]
    M = T * topk
    gs = (0.37 * 1.9 ** (torch.arange(E) % 6) * (1.0 + torch.arange(E) / 4096.0)).float().to(dev)
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}", flush=True)

    for kind in ("uniform", "skewed"):
        if args.quick and kind != "uniform":
            continue
        ids = torch.from_numpy(topk_ids(T, E, topk, kind)).to(dev)
        src_row, offs, _ = q.moe_sort_fused(ids, E)
        ends = [0] + offs.cpu().tolist()   # the loop's host copy of the boundaries, taken once, outside the timing
        ranges = [(g, a, b) for g, (a, b) in enumerate(zip(ends, ends[1:])) if b > a]
        src_of = [src_row[a:b].contiguous() for _, a, b in ranges]
        gs_of = [gs[g:g + 1].contiguous() for g, _, _ in ranges]
        nbuf = int(min(40, max(3, -(-(5 << 28) // (M * H * 2)))))
        xs = [(torch.randn(T, H, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nbuf)]
        for rot in ROTS:
            h = _hadamard(rot, dev)
            forms = {"grouped": lambda j: q.fusedGatherQuantizeNvGrouped(xs[j], h, gs, src_row, offs),
                     "single": lambda j: q.fusedGatherQuantizeNv(xs[j], h, gs_of[0], src_row),
                     "loop": lambda j: [q.fusedGatherQuantizeNv(xs[j], h, s, r) for s, r in zip(gs_of, src_of)]}
            for cache in ("warm", "cold"):
                t = (lambda f: time_us(lambda: f(0), args.iters)) if cache == "warm" else (lambda f: time_us_cold(f, nbuf, max(args.iters // 4, 2 * nbuf)))
                times = {k: [] for k in forms}
                for _ in range(max(1, args.repeat)):
                    for k, f in forms.items():
                        times[k].append(t(f))
                med = {k: float(np.median(v)) for k, v in times.items()}
                spread = (max(times["grouped"]) - min(times["grouped"])) / med["grouped"]
                print(f"gscale {model:14s} {phase:8s} {kind:8s} T={T:5d} M={M:6d} H={H:5d} E={E:4d} live={len(ranges):4d} R={rot:3d} {cache:>5s} grouped_us {med['grouped']:9.2f} "
                      f"single_us {med['single']:9.2f} loop_us {med['loop']:9.2f} grouped/single {med['grouped'] / med['single']:5.3f} loop/grouped {med['loop'] / med['grouped']:6.2f} "
                      f"spread {spread:5.3f}", flush=True)
                print("JSON " + json.dumps(dict(op="gather_quantize_nv_grouped", model=model, phase=phase, routing=kind, T=T, M=M, H=H, E=E, live=len(ranges), rot=rot, cache=cache,
                                                grouped_us=round(med["grouped"], 3), single_us=round(med["single"], 3), loop_us=round(med["loop"], 3),
                                                spread=round(spread, 4))), flush=True)
        del xs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (the three forms alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one (model, phase) step may take")
    ap.add_argument("--step", type=int, default=-1, help=argparse.SUPPRESS)   # (internal: run this one step in this process)
    args = ap.parse_args()
    if args.step >= 0:
        run_step(*STEPS[args.step], args)
        return 0
    for i, (m, phase) in enumerate(STEPS):
        if args.quick and phase != "decode":
            continue
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
