#!/usr/bin/env python3
"""The two ends of a mixture-of-experts MLP around the grouped GEMMs, each against the composition it replaces.

  dispatch   fused_us   one launch: fusedGatherQuantize{Mx,Nv}(x, h, src_row)
             lib2_us    the library's own two steps: x.index_select(0, src_row) -> fusedQuantize{Mx,Nv}(xg, h)
             TB/s       bytes the fused op has to move (2 B per routed element in + codes + scales + 4 B per index) / fused time
  combine    fused_us   one launch: moe_combine(y, pos, weights)
             torch_us   the torch composition: (y[pos.clamp(min=0)].float() * (weights * (pos >= 0)).unsqueeze(-1)).sum(1).to(bf16)
             TB/s       bytes moe_combine has to move (2 B per routed element in, 2 B per output element out) / fused time
  spread     (max - min) / median of the fused time over --repeat whole measurements of the row (fused and composed forms alternate)

Timing as bench_configs.py times the streaming ops: medians of HIP-graph replays, WARM (one input replayed: the Infinity Cache serves what fits) and COLD (inputs
rotated so that a cycle exceeds 1 GiB -- or 40 inputs of a small shape).

Shapes: the layers and routings of benchmarks/bench_grouped_mxfp4_mi355x.py -- Qwen3-30B-A3B (H = 2048, E = 128, top-8) and Mixtral-8x7B (H = 4096, E = 8, top-2) at
decode (64 tokens) and prefill (4096 tokens), uniform and skewed routing (half of the routed rows in one expert); MX at R = 32 and 128, NV at R = 16.

Every (model, phase) is one GPU step: a child process of its own under its own time limit (--step-timeout), and the first step that fails or runs out of time ends the
run -- nothing more is started on a device that has just misbehaved.

    python benchmarks/bench_moe_dispatch_mi355x.py [--repeat 3] [--quick] [--step-timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (model, H, E, top-k)
MODELS = [("Qwen3-30B-A3B", 2048, 128, 8), ("Mixtral-8x7B", 4096, 8, 2)]
TOKENS = {"decode": 64, "prefill": 4096}
FORMATS = [("mx", 32), ("mx", 128), ("nv", 16)]
STEPS = [(m, p) for m in range(len(MODELS)) for p in TOKENS]


def _hadamard(n, dev):
    import torch

    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(dev)


def topk_ids(T, E, topk, kind, seed=0):
    """router output (T, topk): uniform -- top-k distinct experts per token; skewed -- then half of all slots, picked at random, are sent to expert 0"""
    import numpy as np

    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(E)[:topk] for _ in range(T)])
    if kind == "skewed":   # half of the routed rows go to expert 0 (as the grouped benchmarks' skewed routing)
        flat = ids.reshape(-1)
        flat[rng.permutation(flat.size)[: flat.size // 2]] = 0
    return ids


def run_step(model_i, phase, args):
    import numpy as np
    import torch

    from bench_configs import time_us, time_us_cold
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    model, H, E, topk = MODELS[model_i]
    T = TOKENS[phase]
    M = T * topk
    gs = torch.tensor([3.0], device=dev)
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}", flush=True)

    def measure(fa, fb, nbuf):
        """(warm, cold) x (median a, median b, spread of a): a and b alternate inside every repeat"""
        res = {}
        for cache in ("warm", "cold"):
            t = (lambda f: time_us(lambda: f(0), args.iters)) if cache == "warm" else (lambda f: time_us_cold(f, nbuf, max(args.iters // 4, 2 * nbuf)))
            ta, tb = [], []
            for _ in range(max(1, args.repeat)):
                ta.append(t(fa))
                tb.append(t(fb))
            a_, b_ = float(np.median(ta)), float(np.median(tb))
            res[cache] = (a_, b_, (max(ta) - min(ta)) / a_)
        return res

    for kind in ("uniform", "skewed"):
        if args.quick and kind != "uniform":
            continue
        ids = torch.from_numpy(topk_ids(T, E, topk, kind)).to(dev)
        src_row, offs, pos = q.moe_sort(ids, E)
        src_long = src_row.long()
        # ---- dispatch: the token matrix is what rotates (x is read through the index, T * H * 2 bytes); a cold cycle reads > 1.25 GiB of routed rows or 40 inputs
        nbuf = int(min(40, max(3, -(-(5 << 28) // (M * H * 2)))))
        xs = [(torch.randn(T, H, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nbuf)]
        for fmt, rot in FORMATS:
            h = _hadamard(rot, dev)
            if fmt == "mx":
                fused = lambda j: q.fusedGatherQuantizeMx(xs[j], h, src_row, method="abs_max")
                lib2 = lambda j: q.fusedQuantizeMx(xs[j].index_select(0, src_long), h, method="abs_max")
            else:
                fused = lambda j: q.fusedGatherQuantizeNv(xs[j], h, gs, src_row)
                lib2 = lambda j: q.fusedQuantizeNv(xs[j].index_select(0, src_long), h, gs)
            moved = M * H * 2 + M * H // 2 + M * H // (32 if fmt == "mx" else 16) + M * 4
            for cache, (f_, l_, spread) in measure(fused, lib2, nbuf).items():
                print(f"dispatch {model:14s} {phase:8s} {kind:8s} T={T:5d} M={M:6d} H={H:5d} {fmt:>3s} R={rot:3d} {cache:>5s} fused_us {f_:9.2f} lib2_us {l_:9.2f} "
                      f"lib2/fused {l_ / f_:5.2f} TB/s {moved / f_ / 1e6:6.2f} spread {spread:5.3f}", flush=True)
                print("JSON " + json.dumps(dict(op="dispatch", model=model, phase=phase, routing=kind, T=T, M=M, H=H, fmt=fmt, rot=rot, cache=cache, fused_us=round(f_, 3),
                                                lib2_us=round(l_, 3), fused_TBps=round(moved / f_ / 1e6, 3), spread=round(spread, 4))), flush=True)
        del xs
        # ---- combine: y (M, H) rotates
        ys = [torch.randn(M, H, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        w = torch.softmax(torch.randn(T, topk, device=dev), dim=-1)
        posc, wz = pos.clamp(min=0).long(), (w * (pos >= 0)).unsqueeze(-1)
        fused = lambda j: q.moe_combine(ys[j], pos, w)
        tor = lambda j: (ys[j][posc].float() * wz).sum(1).to(torch.bfloat16)
        moved = M * H * 2 + T * H * 2 + M * 8
        for cache, (f_, t_, spread) in measure(fused, tor, nbuf).items():
            print(f"combine  {model:14s} {phase:8s} {kind:8s} T={T:5d} M={M:6d} H={H:5d} {'':>3s} {'':5s} {cache:>5s} fused_us {f_:9.2f} torch_us {t_:8.2f} "
                  f"torch/fused {t_ / f_:4.2f} TB/s {moved / f_ / 1e6:6.2f} spread {spread:5.3f}", flush=True)
            print("JSON " + json.dumps(dict(op="combine", model=model, phase=phase, routing=kind, T=T, M=M, H=H, topk=topk, cache=cache, fused_us=round(f_, 3),
                                            torch_us=round(t_, 3), fused_TBps=round(moved / f_ / 1e6, 3), spread=round(spread, 4))), flush=True)
        del ys
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (the fused and the composed form alternate); medians are reported")
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
