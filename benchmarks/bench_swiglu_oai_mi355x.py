#!/usr/bin/env python3
"""The two gpt-oss ops between and behind the grouped GEMMs of an expert layer: the clamped SwiGLU with the gate/up bias fused into the MXFP4 quantizer
(qutlass_amd.fusedSwigluOaiQuantizeMx) and moe_combine with the down bias, against what they replace.

  activation rows (one per shape, R and cache state):
    fused_us     one launch: fusedSwigluOaiQuantizeMx(x, h, bias=b1, offs=offs)
    lib2_us      the library's two launches: swiglu_oai_and_mul(x, bias=b1, offs=offs) -> fusedQuantizeMx(act, h)
    torch_us     the torch composition: x + b1[expert of row] (searchsorted + index_select + add), clamp, sigmoid, multiply -> fusedQuantizeMx(act, h)
    fused0_us    the fused op without a bias;  lib20_us  the two launches without a bias  (fused_us - fused0_us: what the bias costs)
    TB/s         bytes the fused op moves (4 B in + codes + scales per output element; the bias rows come from L2) / fused time
    spread       (max - min) / median of fused_us over --repeat whole measurements of the row
  combine rows (one per shape and cache state):
    bias_us      moe_combine(y, pos, weights, bias=b2, offs=offs)
    torch_us     y + b2[expert of row] -> moe_combine
    plain_us     moe_combine(y, pos, weights)            (bias_us - plain_us: what the bias costs)

Timing as bench_gated_quantize_mi355x.py: medians of HIP-graph replays, WARM (one input replayed) and COLD (inputs rotated so that a cycle exceeds 1 GiB).

Shapes: gpt-oss-20b (E 32, top-4) and gpt-oss-120b (E 128, top-4), I = H = 2944 (2880 padded to a multiple of 128), 16 / 128 / 4096 tokens -- rows = 4 x tokens,
dealt to the experts at random.

    python benchmarks/bench_swiglu_oai_mi355x.py [--repeat 3] [--quick]
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

MODELS = [("gpt-oss-20b", 32, 4), ("gpt-oss-120b", 128, 4)]
TOKENS = [16, 128, 4096]
WIDTH = 2944
ALPHA, LIMIT = 1.702, 7.0


def _hadamard(n, dev):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (the configurations alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="16 and 128 tokens only")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}")
    gen = torch.Generator(device="cpu").manual_seed(0)
    inter = hid = WIDTH

    def med(fs, cache, xs):
        """medians of the alternating measurements of the callables fs (each takes one input)"""
        def t(f):
            return time_us(lambda: f(xs[0]), args.iters) if cache == "warm" else time_us_cold(lambda j: f(xs[j]), len(xs), max(args.iters // 4, 2 * len(xs)))
        runs = [[t(f) for f in fs] for _ in range(max(1, args.repeat))]
        cols = list(zip(*runs))
        return [float(np.median(c)) for c in cols], (max(cols[0]) - min(cols[0])) / float(np.median(cols[0]))

    print(f"{'op':8s} {'model':13s} {'tokens':>6s} {'rows':>6s} {'R':>3s} {'cache':>5s} {'fused_us':>9s} {'lib2_us':>9s} {'torch_us':>9s} {'fused0_us':>9s} {'lib20_us':>9s} "
          f"{'lib2/f':>6s} {'torch/f':>7s} {'bias':>6s} {'TB/s':>6s} {'spread':>6s}")
    for model, E, topk in MODELS:
        for tokens in TOKENS:
            if args.quick and tokens > 128:
                continue
            rows = tokens * topk
            counts = torch.bincount(torch.randint(0, E, (rows,), generator=gen), minlength=E)
            offs = torch.cumsum(counts, 0).to(torch.int32).to(dev)
            offs64 = offs.to(torch.int64)
            row_ids = torch.arange(rows, device=dev)
            b1 = torch.randn(E, 2 * inter, generator=gen).to(torch.bfloat16).to(dev)
            b2 = torch.randn(E, hid, generator=gen).to(torch.bfloat16).to(dev)
            xbytes = rows * 2 * inter * 2
            nbuf = int(min(40, max(3, -(-(5 << 28) // xbytes))))
            xs = [(torch.randn(rows, 2 * inter, device=dev) * 3.0).to(torch.bfloat16) for _ in range(nbuf)]

            def experts():
                return torch.searchsorted(offs64, row_ids, right=True).clamp_(max=E - 1)

            for rot in (32, 64):
                h = _hadamard(rot, dev)
                plain = lambda a: q.fusedQuantizeMx(a, h, method="abs_max")
                fused = lambda x: q.fusedSwigluOaiQuantizeMx(x, h, alpha=ALPHA, limit=LIMIT, bias=b1, offs=offs, method="abs_max")
                lib2 = lambda x: plain(q.swiglu_oai_and_mul(x, alpha=ALPHA, limit=LIMIT, bias=b1, offs=offs))
                fused0 = lambda x: q.fusedSwigluOaiQuantizeMx(x, h, alpha=ALPHA, limit=LIMIT, method="abs_max")
                lib20 = lambda x: plain(q.swiglu_oai_and_mul(x, alpha=ALPHA, limit=LIMIT))

                def tor(x):
                    xb = x + b1.index_select(0, experts())
                    g = xb[..., :inter].clamp(max=LIMIT)
                    u = xb[..., inter:].clamp(-LIMIT, LIMIT)
                    return plain((u + 1) * (g * torch.sigmoid(g * ALPHA)))

                obytes = rows * inter // 2 + rows * inter // 32
                for cache in ("warm", "cold"):
                    (f_, l_, t_, f0, l0), spread = med([fused, lib2, tor, fused0, lib20], cache, xs)
                    tbps = (xbytes + obytes) / f_ / 1e6
                    print(f"{'act+q':8s} {model:13s} {tokens:6d} {rows:6d} {rot:3d} {cache:>5s} {f_:9.2f} {l_:9.2f} {t_:9.2f} {f0:9.2f} {l0:9.2f} {l_ / f_:6.2f} {t_ / f_:7.2f} "
                          f"{f_ - f0:6.2f} {tbps:6.2f} {spread:6.3f}", flush=True)
                    print("JSON " + json.dumps(dict(op="swiglu_oai_quantize_mx", model=model, E=E, tokens=tokens, rows=rows, inter=inter, rot=rot, cache=cache,
                                                    fused_us=round(f_, 3), lib2_us=round(l_, 3), torch_us=round(t_, 3), fused_nobias_us=round(f0, 3),
                                                    lib2_nobias_us=round(l0, 3), fused_TBps=round(tbps, 3), spread=round(spread, 4))), flush=True)
            del xs
            # combine: y (rows, H), every row named once
            ybytes = rows * hid * 2
            nbuf = int(min(40, max(3, -(-(5 << 28) // ybytes))))
            ys = [torch.randn(rows, hid, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
            pos = torch.randperm(rows, generator=gen).to(torch.int32).view(tokens, topk).to(dev)
            w = torch.softmax(torch.randn(tokens, topk, generator=gen), dim=-1).to(dev)
            cb = lambda y: q.moe_combine(y, pos, w, bias=b2, offs=offs)
            ct = lambda y: q.moe_combine(y + b2.index_select(0, experts()), pos, w)
            cp = lambda y: q.moe_combine(y, pos, w)
            for cache in ("warm", "cold"):
                (b_, t_, p_), spread = med([cb, ct, cp], cache, ys)
                print(f"{'combine':8s} {model:13s} {tokens:6d} {rows:6d} {'-':>3s} {cache:>5s}  bias_us {b_:8.2f}  torch_us {t_:8.2f}  plain_us {p_:8.2f}  torch/bias {t_ / b_:5.2f}  "
                      f"bias cost {b_ - p_:6.2f}  spread {spread:5.3f}", flush=True)
                print("JSON " + json.dumps(dict(op="moe_combine_bias", model=model, E=E, tokens=tokens, rows=rows, hidden=hid, cache=cache, bias_us=round(b_, 3),
                                                torch_us=round(t_, 3), plain_us=round(p_, 3), spread=round(spread, 4))), flush=True)
            del ys
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
