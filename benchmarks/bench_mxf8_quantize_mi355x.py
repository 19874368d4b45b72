#!/usr/bin/env python3
"""The MXFP8 rotate-and-quantize ops (qutlass_amd.fusedQuantizeMxf8 and its gathering and gated forms), float8_e4m3fn, R = 32 and 128, each against its yardstick:

    plain    new_us   fusedQuantizeMxf8(x, h)                         ref_us   fusedQuantizeMx(x, h, method="abs_max") on the same input
             -- the MXFP4 quantizer moves 2 + 0.53 B per element, this one 2 + 1.03: the byte ratio 3.03 / 2.53 = 1.20 is what new / ref should be if both are HBM-bound
    gather   new_us   fusedGatherQuantizeMxf8(x, h, src_row)          ref_us   x.index_select(0, src_row) -> fusedQuantizeMxf8
    gated    new_us   fusedSiluMulQuantizeMxf8(x, h)                  ref_us   silu_and_mul(x) -> fusedQuantizeMxf8
             -- a fused form that is slower than its two launches (ref/new < 1) is said so in the wrapper's docstring
    TB/s     bytes the new op has to move / new time (plain: 2 B in + 1 B + 1/32 B out per element; gather: + 4 B per index; gated: 4 B in)
    spread   (max - min) / median of new_us over --repeat whole measurements of the row (new and ref alternate inside every repeat): the session's run-to-run spread

Timing as bench_configs.py times the streaming ops: medians of HIP-graph replays, WARM (one input replayed: the Infinity Cache serves what fits) and COLD (inputs
rotated so that a cycle exceeds 1 GiB -- or 40 inputs of a small shape).

Shapes (rows, K) of the quantized operand: 4096^2 and 8192^2, the routed-token matrices of benchmarks/bench_moe_dispatch_mi355x.py -- Qwen3-30B-A3B (H = 2048, top-8)
and Mixtral-8x7B (H = 4096, top-2) at decode (64 tokens) and prefill (4096 tokens), uniform routing -- and 128 x 14336.  gather runs on the four token shapes
(x is (tokens, H)), gated on those and on 128 x 14336 (x is (rows, 2 K)).

    python benchmarks/bench_mxf8_quantize_mi355x.py [--repeat 3] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_configs import time_us, time_us_cold  # noqa: E402

# (name, rows, K, tokens or None): tokens = rows of the token matrix the gathering form reads (rows = tokens * top-k)
SHAPES = [("4096^2", 4096, 4096, None), ("8192^2", 8192, 8192, None), ("Qwen3-30B-A3B decode", 512, 2048, 64), ("Qwen3-30B-A3B prefill", 32768, 2048, 4096),
          ("Mixtral-8x7B decode", 128, 4096, 64), ("Mixtral-8x7B prefill", 8192, 4096, 4096), ("128x14336", 128, 14336, None)]
ROTS = (32, 128)


def _hadamard(n, dev):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (new and ref alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="the decode shapes and 128 x 14336 only")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}  dtype=float8_e4m3fn")
    print(f"{'form':6s} {'shape':22s} {'rows':>6s} {'K':>6s} {'R':>4s} {'cache':>5s} {'new_us':>9s} {'ref_us':>9s} {'new/ref':>7s} {'ref/new':>7s} {'TB/s':>6s} {'spread':>6s}")

    def measure(form, name, rows, k, rot, new, ref, nbuf, moved):
        for cache in ("warm", "cold"):
            t = (lambda f: time_us(lambda: f(0), args.iters)) if cache == "warm" else (lambda f: time_us_cold(f, nbuf, max(args.iters // 4, 2 * nbuf)))
            tn, tr = [], []
            for _ in range(max(1, args.repeat)):
                tn.append(t(new))
                tr.append(t(ref))
            n_, r_ = float(np.median(tn)), float(np.median(tr))
            spread = (max(tn) - min(tn)) / n_
            print(f"{form:6s} {name:22s} {rows:6d} {k:6d} {rot:4d} {cache:>5s} {n_:9.2f} {r_:9.2f} {n_ / r_:7.2f} {r_ / n_:7.2f} {moved / n_ / 1e6:6.2f} {spread:6.3f}", flush=True)
            print("JSON " + json.dumps(dict(form=form, shape=name, rows=rows, k=k, rot=rot, cache=cache, new_us=round(n_, 3), ref_us=round(r_, 3), new_over_ref=round(n_ / r_, 4),
                                            new_TBps=round(moved / n_ / 1e6, 3), spread=round(spread, 4), ref_spread=round((max(tr) - min(tr)) / r_, 4))), flush=True)

    for name, rows, k, tokens in SHAPES:
        if args.quick and not ("decode" in name or name == "128x14336"):
            continue
        numel = rows * k
        out_bytes = numel + numel // 32
        nbuf = int(min(40, max(3, -(-(5 << 28) // (numel * 2)))))          # a cold cycle reads > 1.25 GiB (or 40 inputs of a small shape)
        xs = [(torch.randn(rows, k, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nbuf)]
        for rot in ROTS:
            h = _hadamard(rot, dev)
            measure("plain", name, rows, k, rot, lambda j: q.fusedQuantizeMxf8(xs[j], h), lambda j: q.fusedQuantizeMx(xs[j], h, method="abs_max"), nbuf, numel * 2 + out_bytes)
        del xs
        torch.cuda.empty_cache()
        if tokens is not None:   # the gathering form: uniform routing, every token top-k times, sorted by expert (a random permutation of the slots stands for it)
            src = torch.from_numpy(np.random.default_rng(0).permutation(rows) % tokens).to(torch.int32).to(dev)
            src_long = src.long()
            xt = [(torch.randn(tokens, k, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nbuf)]
            for rot in ROTS:
                h = _hadamard(rot, dev)
                measure("gather", name, rows, k, rot, lambda j: q.fusedGatherQuantizeMxf8(xt[j], h, src), lambda j: q.fusedQuantizeMxf8(xt[j].index_select(0, src_long), h), nbuf,
                        numel * 2 + out_bytes + rows * 4)
            del xt
            torch.cuda.empty_cache()
        if tokens is not None or name == "128x14336":   # the gated form: x is (rows, 2 K)
            nb2 = int(min(40, max(3, -(-(5 << 28) // (numel * 4)))))
            xg = [(torch.randn(rows, 2 * k, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nb2)]
            for rot in ROTS:
                h = _hadamard(rot, dev)
                measure("gated", name, rows, k, rot, lambda j: q.fusedSiluMulQuantizeMxf8(xg[j], h), lambda j: q.fusedQuantizeMxf8(q.silu_and_mul(xg[j]), h), nb2,
                        numel * 4 + out_bytes)
            del xg
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
