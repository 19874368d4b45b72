#!/usr/bin/env python3
"""W4A6 grouped GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf6_mxf4_bf16_tn: MXFP6 e2m3 tokens against MXFP4 expert weights) and its two
quantizers against the paths an MXFP4 checkpoint has without them, on the same expert weights and routing.  Every ratio is time of the alternative / time of this
op: above 1 the new path is faster.

    w4a6_us      the op, the form its rule picks (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays; q20 / q80 beside it)
    w4a6_2_us    the same measurement taken a second time after the other columns: the run-to-run spread of this table
    (a) x8       grouped_matmul_mxf8_mxf4_bf16_tn (W4A8) on tokens of the same shape in e4m3 / w4a6_us
    (b) x4       grouped_matmul_mxf4_bf16_tn (W4A4) / w4a6_us
    (c) xc       (fusedGatherQuantizeMxf8 + W4A8) / (fusedGatherQuantizeMxf6 + this op): the dispatch and the GEMM together, one graph each
    (d) xq, xg   fusedQuantizeMxf8 / fusedQuantizeMxf6 on the (M, K) routed tokens, fusedGatherQuantizeMxf8 / fusedGatherQuantizeMxf6 on the (T, K) tokens (R = 32)
    --forms      also every form of the op forced through the lab library (610 = 32x32, 611 = 32x16, 612 = 64x32): the calibration of the form rule
                 (qutlass_amd/csrc/capi.hip grouped_w4a6_plan)

Shapes: the decode (64 tokens) and prefill (4096 tokens) gate/up and down projections of Qwen3-30B-A3B, Mixtral-8x7B, gpt-oss-20b and gpt-oss-120b, uniform and
skewed routing (benchmarks/bench_grouped_w4a8_mi355x.py).  GEMM operands are random codes with scale bytes near 127, the quantizers' inputs Gaussian (timing only).

    --sweep      instead of the models: 128 experts, N = 2048, a mean of 16 ... 128 rows per expert at K = 768 ... 3712 -- where the rule's thresholds lie

    python benchmarks/bench_grouped_w4a6_mi355x.py [--reps 50] [--forms] [--quick] [--only SUBSTRING] [--sweep]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

_spec = importlib.util.spec_from_file_location("bench_grouped_w4a8_mi355x", os.path.join(ROOT, "benchmarks", "bench_grouped_w4a8_mi355x.py"))
_g8 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_g8)
bench_graph, TOKENS, routing, LAYERS, _fp8 = _g8.bench_graph, _g8.TOKENS, _g8.routing, _g8.LAYERS, _g8._fp8

FORMS = (610, 611, 612)
SWEEP_ROWS, SWEEP_K = (16, 32, 48, 64, 128), (768, 1024, 1536, 2048, 2944, 3712)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--sweep", action="store_true", help="rows per expert x K around the form rule's thresholds instead of the models (GEMM columns only)")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    plans = {}
    for name in ("mxf6_mxf4", "mxf8_mxf4", ""):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_grouped_{name + '_' if name else ''}plan")
        fp.restype = ctypes.c_int
        fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = (f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'w4a6_us':>9s} {'q20':>8s} {'q80':>8s} {'w4a6_2_us':>9s} "
           f"{'f8':>4s} {'w4a8_us':>9s} {'x8':>6s} {'f4':>4s} {'w4a4_us':>9s} {'x4':>6s} {'gq6+6_us':>9s} {'gq8+8_us':>9s} {'xc':>6s} {'q6_us':>8s} {'q8_us':>8s} {'xq':>6s} "
           f"{'gq6_us':>8s} {'gq8_us':>8s} {'xg':>6s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    layers = [("sweep", f"K{K}", 128, 2048, K, 1) for K in SWEEP_K] if args.sweep else LAYERS
    tokens = {f"r{r}": 128 * r for r in SWEEP_ROWS} if args.sweep else TOKENS
    eye = torch.eye(32, dtype=torch.bfloat16, device=dev)
    for model, proj, E, N, K, topk in layers:
        if args.only and args.only not in model:
            continue
        kb = K // 32
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = torch.randint(124, 131, (E * N * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        for phase, T in tokens.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            a6 = torch.randint(0, 256, (M, K * 3 // 4), dtype=torch.uint8, device=dev, generator=gen)   # every byte string is 6-bit codes: the format has no NaN
            a8 = _fp8((M, K), dev, gen)
            a4 = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=gen)
            a_sf = torch.randint(124, 131, (M * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
            alpha = torch.ones(1, device=dev)
            x = torch.randn(T, K, dtype=torch.bfloat16, device=dev, generator=gen)
            src = (torch.arange(M, device=dev, dtype=torch.int32) * 7919 % T).to(torch.int32)   # every token topk times, in a scattered order
            xs = x.index_select(0, src.long())
            for kind in ("uniform", "skewed"):
                if (args.quick or args.sweep) and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)

                def w4a6():
                    q.grouped_matmul_mxf6_mxf4_bf16_tn(a6, b4, a_sf, b_sf, alpha, offs)

                def w4a8():
                    q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b4, a_sf, b_sf, alpha, offs)

                def w4a4():
                    q.grouped_matmul_mxf4_bf16_tn(a4, b4, a_sf, b_sf, alpha, offs)

                def chain6():
                    c6, s6 = q.fusedGatherQuantizeMxf6(x, eye, src)
                    q.grouped_matmul_mxf6_mxf4_bf16_tn(c6, b4, s6, b_sf, alpha, offs)

                def chain8():
                    c8, s8 = q.fusedGatherQuantizeMxf8(x, eye, src)
                    q.grouped_matmul_mxf8_mxf4_bf16_tn(c8, b4, s8, b_sf, alpha, offs)

                t, lo, hi = (v * 1e3 for v in bench_graph(w4a6, args.reps)[:3])
                t8 = bench_graph(w4a8, args.reps)[0] * 1e3
                t4 = bench_graph(w4a4, args.reps)[0] * 1e3
                tc6 = tc8 = tq6 = tq8 = tg6 = tg8 = float("nan")
                if not args.sweep:
                    tc6 = bench_graph(chain6, args.reps)[0] * 1e3
                    tc8 = bench_graph(chain8, args.reps)[0] * 1e3
                    if kind == "uniform":   # the quantizers do not see the routing
                        tq6 = bench_graph(lambda: q.fusedQuantizeMxf6(xs, eye), args.reps)[0] * 1e3
                        tq8 = bench_graph(lambda: q.fusedQuantizeMxf8(xs, eye), args.reps)[0] * 1e3
                        tg6 = bench_graph(lambda: q.fusedGatherQuantizeMxf6(x, eye, src), args.reps)[0] * 1e3
                        tg8 = bench_graph(lambda: q.fusedGatherQuantizeMxf8(x, eye, src), args.reps)[0] * 1e3
                ft = {}
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    for v in FORMS:
                        def forced():
                            f(a6.data_ptr(), b4.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), out.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(w4a6, args.reps)[0] * 1e3
                form, f8, f4 = (str(plans[n](M, N, K, E, None)) for n in ("mxf6_mxf4", "mxf8_mxf4", ""))
                line = (f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {t2:9.2f} {f8:>4s} {t8:9.2f} {t8 / t:6.2f} "
                        f"{f4:>4s} {t4:9.2f} {t4 / t:6.2f} {tc6:9.2f} {tc8:9.2f} {tc8 / tc6:6.2f} {tq6:8.2f} {tq8:8.2f} {tq8 / tq6:6.2f} {tg6:8.2f} {tg8:8.2f} {tg8 / tg6:6.2f}")
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, w4a6_us=round(t, 3), w4a6_q20_us=round(lo, 3), w4a6_q80_us=round(hi, 3),
                           w4a6_again_us=round(t2, 3), w4a8_form=f8, w4a8_us=round(t8, 3), w4a4_form=f4, w4a4_us=round(t4, 3), gather6_w4a6_us=round(tc6, 3),
                           gather8_w4a8_us=round(tc8, 3), quantize6_us=round(tq6, 3), quantize8_us=round(tq8, 3), gather6_us=round(tg6, 3), gather8_us=round(tg8, 3))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(v_us, 3) for v, v_us in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps({k: None if isinstance(v, float) and v != v else v for k, v in rec.items()}), flush=True)
            del a6, a8, a4, a_sf, x, xs, src
        del b4, b_sf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
