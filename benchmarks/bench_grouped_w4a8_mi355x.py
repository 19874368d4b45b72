#!/usr/bin/env python3
"""W4A8 grouped GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf8_mxf4_bf16_tn: MXFP8 tokens against MXFP4 expert weights) against the two ways
to run an MXFP4 checkpoint without it, on the same tokens, expert weights and routing:

    w4a8_us      the op, the form its rule picks (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays; q20 / q80 beside it)
    w4a8_2_us    the same measurement taken a second time after the other columns: the run-to-run spread of this table
    mxf8_up_us   grouped_matmul_mxf8_bf16_tn on the weights upcast to e4m3 -- the same numerics, twice the weight bytes (the upcast is outside the timed region)
    mxf4_us      grouped_matmul_mxf4_bf16_tn on 4-bit tokens -- the same weight bytes, W4A4 numerics
    x8 / x4      mxf8_up_us / w4a8_us and mxf4_us / w4a8_us: above 1 the new op is faster
    --forms      also every form of the op forced through the lab library (602 = 32x32, 603 = 32x16, 604 = 64x32): the calibration of the form rule
                 (qutlass_amd/csrc/capi.hip grouped_w4a8_plan)

Shapes: the decode (64 tokens) and prefill (4096 tokens) gate/up and down projections of Qwen3-30B-A3B and Mixtral-8x7B (benchmarks/bench_grouped_mxfp4_mi355x.py)
and of gpt-oss-20b / gpt-oss-120b (32 / 128 experts, top-4) with I = H = 2944 (2880 padded to the ops' K % 128 == 0).  Operands are random codes (NaN codes
replaced) with scale bytes near 127 (timing only).

    --sweep      instead of the models: 128 experts, N = 2048, a mean of 16 ... 128 rows per expert at K = 768 ... 2944 -- where the rule's two thresholds lie

    python benchmarks/bench_grouped_w4a8_mi355x.py [--reps 50] [--forms] [--quick] [--only SUBSTRING] [--sweep]
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

_spec = importlib.util.spec_from_file_location("bench_grouped_mxfp4_mi355x", os.path.join(ROOT, "benchmarks", "bench_grouped_mxfp4_mi355x.py"))
_g4 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_g4)
bench_graph, TOKENS, routing = _g4.bench_graph, _g4.TOKENS, _g4.routing

LAYERS = list(_g4.LAYERS) + [
    ("gpt-oss-20b", "gate_up", 32, 2 * 2944, 2944, 4),
    ("gpt-oss-20b", "down", 32, 2944, 2944, 4),
    ("gpt-oss-120b", "gate_up", 128, 2 * 2944, 2944, 4),
    ("gpt-oss-120b", "down", 128, 2944, 2944, 4),
]
FORMS = (602, 603, 604)
SWEEP_ROWS, SWEEP_K = (16, 32, 48, 64, 128), (768, 1024, 1280, 1536, 2048, 2944)
E2M1_AS_E4M3 = [0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C, 0x80, 0xB0, 0xB8, 0xBC, 0xC0, 0xC4, 0xC8, 0xCC]   # e2m1 code -> the e4m3 byte of the same value


def _fp8(shape, dev, gen):
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)
    x[(x & 0x7F) == 0x7F] = 0x7E   # no NaN codes
    return x.view(torch.float8_e4m3fn)


def _upcast(b4):
    """(E, N, K/2) packed e2m1 -> (E, N, K) e4m3, expert by expert (the index tensors stay small)"""
    lut = torch.tensor(E2M1_AS_E4M3, dtype=torch.uint8, device=b4.device)
    E, N, K2 = b4.shape
    out = torch.empty(E, N, 2 * K2, dtype=torch.uint8, device=b4.device)
    for g in range(E):
        out[g, :, 0::2] = lut[(b4[g] & 0xF).long()]
        out[g, :, 1::2] = lut[(b4[g] >> 4).long()]
    return out.view(torch.float8_e4m3fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--sweep", action="store_true", help="rows per expert x K around the form rule's thresholds instead of the models")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    plans = {}
    for name in ("mxf8_mxf4", "mxf8", ""):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_grouped_{name + '_' if name else ''}plan")
        fp.restype = ctypes.c_int
        fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = (f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'w4a8_us':>9s} {'q20':>8s} {'q80':>8s} {'w4a8_2_us':>9s} "
           f"{'f8':>4s} {'mxf8_up_us':>10s} {'x8':>6s} {'f4':>4s} {'mxf4_us':>9s} {'x4':>6s} {'TB/s':>6s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    layers = [("sweep", f"K{K}", 128, 2048, K, 1) for K in SWEEP_K] if args.sweep else LAYERS
    tokens = {f"r{r}": 128 * r for r in SWEEP_ROWS} if args.sweep else TOKENS
    for model, proj, E, N, K, topk in layers:
        if args.only and args.only not in model:
            continue
        kb = K // 32
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b8 = _upcast(b4)
        b_sf = torch.randint(124, 131, (E * N * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        for phase, T in tokens.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            a8 = _fp8((M, K), dev, gen)
            a4 = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=gen)
            a_sf = torch.randint(124, 131, (M * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
            alpha = torch.ones(1, device=dev)
            for kind in ("uniform", "skewed"):
                if (args.quick or args.sweep) and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)
                live = int((c > 0).sum())

                def w4a8():
                    q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b4, a_sf, b_sf, alpha, offs)

                def mxf8_up():
                    q.grouped_matmul_mxf8_bf16_tn(a8, b8, a_sf, b_sf, alpha, offs)

                def mxf4():
                    q.grouped_matmul_mxf4_bf16_tn(a4, b4, a_sf, b_sf, alpha, offs)

                t, lo, hi = (x * 1e3 for x in bench_graph(w4a8, args.reps)[:3])
                t8 = bench_graph(mxf8_up, args.reps)[0] * 1e3
                t4 = bench_graph(mxf4, args.reps)[0] * 1e3
                ft = {}
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    for v in FORMS:
                        def forced():
                            f(a8.data_ptr(), b4.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), out.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(w4a8, args.reps)[0] * 1e3
                wbytes = live * N * (K // 2 + kb)
                form, f8, f4 = (str(plans[n](M, N, K, E, None)) for n in ("mxf8_mxf4", "mxf8", ""))
                line = (f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {t2:9.2f} {f8:>4s} {t8:10.2f} {t8 / t:6.2f} "
                        f"{f4:>4s} {t4:9.2f} {t4 / t:6.2f} {wbytes / t / 1e6:6.2f}")
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, w4a8_us=round(t, 3), w4a8_q20_us=round(lo, 3), w4a8_q80_us=round(hi, 3),
                           w4a8_again_us=round(t2, 3), mxf8_form=f8, mxf8_upcast_us=round(t8, 3), mxf4_form=f4, mxf4_us=round(t4, 3), weight_TBps=round(wbytes / t / 1e6, 3))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(x, 3) for v, x in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del a8, a4, a_sf
        del b4, b8, b_sf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
