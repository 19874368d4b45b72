#!/usr/bin/env python3
"""The activation of a gpt-oss W4A8 expert layer (MXFP4 weights as stored, 8-bit tokens: grouped_matmul_mxf8_mxf4_bf16_tn on both sides): the clamped SwiGLU with
the gate/up bias fused into the MXFP8 quantizer (qutlass_amd.fusedSwigluOaiQuantizeMxf8), against what it replaces.

  one row per shape, R and cache state:
    fused_us     one launch: fusedSwigluOaiQuantizeMxf8(x, h, bias=b1, offs=offs)
    lib2_us      the library's two launches: swiglu_oai_and_mul(x, bias=b1, offs=offs) -> fusedQuantizeMxf8(act, h)
    torch_us     the torch composition: x + b1[expert of row] (searchsorted + index_select + add), clamp, sigmoid, multiply -> fusedQuantizeMxf8(act, h)
    mx4_us       fusedSwigluOaiQuantizeMx(x, h, bias=b1, offs=offs, method="abs_max") on the same input: the byte-ratio yardstick (4.53 B moved per output
                 element against 5.03 B here: the same reads, half the code bytes)
    TB/s         bytes the fused op moves (4 B in + 1 B code + 1/32 B scale per output element; the bias rows come from L2) / fused time
    f_sprd, l_sprd   (max - min) / median of fused_us and of lib2_us over --repeat whole measurements of the row: a ratio inside the two spreads says nothing

Timing as bench_swiglu_oai_mi355x.py: medians of HIP-graph replays, WARM (one input replayed) and COLD (inputs rotated so that a cycle exceeds 1 GiB); the
configurations alternate within a measurement.

Shapes: gpt-oss-20b (E 32, top-4) and gpt-oss-120b (E 128, top-4), I = 2944 (2880 padded to a multiple of 128), 16 / 128 / 4096 tokens -- rows = 4 x tokens,
dealt to the experts at random -- at R = 32 and 64.

    python benchmarks/bench_swiglu_oai_mxf8_mi355x.py [--repeat 3] [--quick]
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
    inter = WIDTH

    def med(fs, cache, xs):
        """medians of the alternating measurements of the callables fs (each takes one input), and the spread of each"""
        def t(f):
            return time_us(lambda: f(xs[0]), args.iters) if cache == "warm" else time_us_cold(lambda j: f(xs[j]), len(xs), max(args.iters // 4, 2 * len(xs)))
        runs = [[t(f) for f in fs] for _ in range(max(1, args.repeat))]
        cols = list(zip(*runs))
        return [float(np.median(c)) for c in cols], [(max(c) - min(c)) / float(np.median(c)) for c in cols]

    print(f"{'model':13s} {'tokens':>6s} {'rows':>6s} {'R':>3s} {'cache':>5s} {'fused_us':>9s} {'lib2_us':>9s} {'torch_us':>9s} {'mx4_us':>9s} {'lib2/f':>6s} {'torch/f':>7s} "
          f"{'f/mx4':>6s} {'TB/s':>6s} {'f_sprd':>6s} {'l_sprd':>6s}")
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
            xbytes = rows * 2 * inter * 2
            nbuf = int(min(40, max(3, -(-(5 << 28) // xbytes))))
            xs = [(torch.randn(rows, 2 * inter, device=dev) * 3.0).to(torch.bfloat16) for _ in range(nbuf)]

            def experts():
                return torch.searchsorted(offs64, row_ids, right=True).clamp_(max=E - 1)

            for rot in (32, 64):
                h = _hadamard(rot, dev)
                plain = lambda a: q.fusedQuantizeMxf8(a, h)
                fused = lambda x: q.fusedSwigluOaiQuantizeMxf8(x, h, alpha=ALPHA, limit=LIMIT, bias=b1, offs=offs)
                lib2 = lambda x: plain(q.swiglu_oai_and_mul(x, alpha=ALPHA, limit=LIMIT, bias=b1, offs=offs))
                mx4 = lambda x: q.fusedSwigluOaiQuantizeMx(x, h, alpha=ALPHA, limit=LIMIT, bias=b1, offs=offs, method="abs_max")

                def tor(x):
                    xb = x + b1.index_select(0, experts())
                    g = xb[..., :inter].clamp(max=LIMIT)
                    u = xb[..., inter:].clamp(-LIMIT, LIMIT)
                    return plain((u + 1) * (g * torch.sigmoid(g * ALPHA)))

                obytes = rows * inter + rows * inter // 32
                for cache in ("warm", "cold"):
                    (f_, l_, t_, m_), (fs_, ls_, _, _) = med([fused, lib2, tor, mx4], cache, xs)
                    tbps = (xbytes + obytes) / f_ / 1e6
                    print(f"{model:13s} {tokens:6d} {rows:6d} {rot:3d} {cache:>5s} {f_:9.2f} {l_:9.2f} {t_:9.2f} {m_:9.2f} {l_ / f_:6.2f} {t_ / f_:7.2f} {f_ / m_:6.2f} "
                          f"{tbps:6.2f} {fs_:6.3f} {ls_:6.3f}", flush=True)
                    print("JSON " + json.dumps(dict(op="swiglu_oai_quantize_mxf8", model=model, E=E, tokens=tokens, rows=rows, inter=inter, rot=rot, cache=cache,
                                                    fused_us=round(f_, 3), lib2_us=round(l_, 3), torch_us=round(t_, 3), mx4_us=round(m_, 3), fused_TBps=round(tbps, 3),
                                                    fused_spread=round(fs_, 4), lib2_spread=round(ls_, 4))), flush=True)
            del xs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
