#!/usr/bin/env python3
"""Activation + quantizer between the two GEMMs of a gated MLP: the fused op (qutlass_amd.fusedSiluMulQuantizeMx / Nv: gate and up read once, the activation in
registers) against the two compositions it replaces.

    fused_us     one launch: fusedSiluMulQuantize{Mx,Nv}(x, h)
    lib2_us      the library's own two launches: silu_and_mul(x) -> fusedQuantize{Mx,Nv}(act, h)
    torch_us     torch's activation: F.silu(x[..., :I]) * x[..., I:] -> fusedQuantize{Mx,Nv}(act, h)
    TB/s         bytes the fused op moves (4 B in + codes + scales per output element) / fused time
    spread       (max - min) / median of the fused time over --repeat whole measurements of the row (the run-to-run spread of the session)

Timing as bench_configs.py times the streaming ops: medians of HIP-graph replays, WARM (one input replayed: the Infinity Cache serves what fits) and COLD (inputs
rotated so that a cycle exceeds 1 GiB).  --per-cu also times the fused op through the lab library with the grid rule's workgroups per CU forced to each listed
value (the calibration of quant_grid for the doubled read stream).

Shapes: Qwen3-30B-A3B (I = 768; decode 64 tokens x top-8 = 512 rows, prefill 32768 rows) and Mixtral-8x7B (I = 14336; 128 and 8192 rows); MX at R = 32 and 128,
NV at R = 16.

    python benchmarks/bench_gated_quantize_mi355x.py [--repeat 3] [--quick] [--per-cu 2,4,8]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_configs import time_us, time_us_cold  # noqa: E402

SHAPES = [("Qwen3-30B-A3B", "decode", 512, 768), ("Qwen3-30B-A3B", "prefill", 32768, 768), ("Mixtral-8x7B", "decode", 128, 14336), ("Mixtral-8x7B", "prefill", 8192, 14336)]
FORMATS = [("mx", 32), ("mx", 128), ("nv", 16)]


def _hadamard(n, dev):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (the three configurations alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="the two decode shapes only")
    ap.add_argument("--per-cu", default="", help="calibration: comma-separated workgroups per CU forced through the lab library (fused op, warm and cold)")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    per_cu = [int(v) for v in args.per_cu.split(",")] if args.per_cu else []
    lab = None
    if per_cu:
        import _benchlib as lab

        fmx = lab.load().qutlass_amd_fused_silu_mul_quantize_mx
        fmx.restype, fmx.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
        fnv = lab.load().qutlass_amd_fused_silu_mul_quantize_nv
        fnv.restype, fnv.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}")
    hdr = f"{'model':14s} {'phase':8s} {'rows':>6s} {'I':>6s} {'fmt':>4s} {'R':>4s} {'cache':>5s} {'fused_us':>9s} {'lib2_us':>9s} {'torch_us':>9s} {'lib2/f':>6s} {'torch/f':>7s} {'TB/s':>6s} {'spread':>6s}"
    if per_cu:
        hdr += "  " + " ".join(f"{'pc' + str(v):>8s}" for v in per_cu)
    print(hdr)
    gs = torch.tensor([3.0], device=dev)
    for model, phase, rows, inter in SHAPES:
        if args.quick and phase != "decode":
            continue
        xbytes = rows * 2 * inter * 2
        nbuf = int(min(40, max(3, -(-(5 << 28) // xbytes))))          # a cold cycle reads > 1.25 GiB (or 40 inputs of a small shape)
        xs = [(torch.randn(rows, 2 * inter, device=dev) * 4.0).to(torch.bfloat16) for _ in range(nbuf)]
        for fmt, rot in FORMATS:
            h = _hadamard(rot, dev)
            if fmt == "mx":
                fused = lambda x: q.fusedSiluMulQuantizeMx(x, h, method="abs_max")
                plain = lambda a: q.fusedQuantizeMx(a, h, method="abs_max")
                obytes = rows * inter // 2 + rows * inter // 32
            else:
                fused = lambda x: q.fusedSiluMulQuantizeNv(x, h, gs)
                plain = lambda a: q.fusedQuantizeNv(a, h, gs)
                obytes = rows * inter // 2 + rows * inter // 16
            lib2 = lambda x: plain(q.silu_and_mul(x))
            tor = lambda x: plain(F.silu(x[..., :inter]) * x[..., inter:])
            out_c = torch.empty(rows, inter // 2, dtype=torch.uint8, device=dev)
            out_s = torch.empty(-(-rows // 128) * 128 * (-(-(inter // 16) // 4) * 4), dtype=torch.uint8, device=dev)

            def forced(x):
                s = torch.cuda.current_stream().cuda_stream
                if fmt == "mx":
                    rc = fmx(x.data_ptr(), h.data_ptr(), rot, rows, inter, 1, 0, out_c.data_ptr(), out_s.data_ptr(), s)
                else:
                    rc = fnv(x.data_ptr(), h.data_ptr(), rot, rows, inter, 1, gs.data_ptr(), 0, out_c.data_ptr(), out_s.data_ptr(), s)
                assert rc == 0

            for cache in ("warm", "cold"):
                def t(f):
                    return time_us(lambda: f(xs[0]), args.iters) if cache == "warm" else time_us_cold(lambda j: f(xs[j]), nbuf, max(args.iters // 4, 2 * nbuf))
                tf, tl, tt = [], [], []
                for _ in range(max(1, args.repeat)):
                    tf.append(t(fused))
                    tl.append(t(lib2))
                    tt.append(t(tor))
                f_, l_, t_ = float(np.median(tf)), float(np.median(tl)), float(np.median(tt))
                spread = (max(tf) - min(tf)) / f_
                tbps = (xbytes + obytes) / f_ / 1e6
                line = f"{model:14s} {phase:8s} {rows:6d} {inter:6d} {fmt:>4s} {rot:4d} {cache:>5s} {f_:9.2f} {l_:9.2f} {t_:9.2f} {l_ / f_:6.2f} {t_ / f_:7.2f} {tbps:6.2f} {spread:6.3f}"
                rec = dict(model=model, phase=phase, rows=rows, inter=inter, fmt=fmt, rot=rot, cache=cache, fused_us=round(f_, 3), lib2_us=round(l_, 3), torch_us=round(t_, 3),
                           fused_TBps=round(tbps, 3), spread=round(spread, 4), lib2_spread=round((max(tl) - min(tl)) / l_, 4))
                if per_cu:
                    pc = {}
                    for v in per_cu:
                        with lab.forced(quant_wg_per_cu=v):
                            pc[v] = t(forced)
                    line += "  " + " ".join(f"{pc[v]:8.2f}" for v in per_cu)
                    rec["per_cu_us"] = {str(v): round(x, 3) for v, x in pc.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
        del xs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
