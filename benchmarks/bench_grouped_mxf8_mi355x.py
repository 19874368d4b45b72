#!/usr/bin/env python3
"""Grouped MXFP8 GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf8_bf16_tn) against the loop it replaces: one matmul_mxf8_bf16_tn per
expert with the group offsets already on the host and every group's to_blocked scales prepared outside the timed region (the loop's best case -- a real
caller pays a device -> host sync for the offsets, one to_blocked per group, and cannot capture the loop).

    grouped_us   one launch over all experts (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays)
    loop_us      E launches of matmul_mxf8_bf16_tn, one per non-empty group, captured into the same kind of graph
    TB/s         bytes of the weights of the non-empty groups (e4m3 + e8m0) / grouped time
    --forms      also every form of the grouped op forced through the lab library (594 = 32x32, 595 = 32x16, 596 = 64x32, 597 = 64x64 ring): the calibration
                 of the form rule (qutlass_amd/csrc/capi.hip grouped8_plan)

Shapes, routings and timing: those of benchmarks/bench_grouped_mxfp4_mi355x.py (Qwen3-30B-A3B and Mixtral-8x7B gate/up and down projections at decode and
prefill, uniform and skewed routing).  Operands are random e4m3 codes (NaN codes replaced) with scale bytes near 127 (timing only).

    python benchmarks/bench_grouped_mxf8_mi355x.py [--reps 50] [--forms] [--quick]
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
bench_graph, LAYERS, TOKENS, routing = _g4.bench_graph, _g4.LAYERS, _g4.TOKENS, _g4.routing

FORMS = (594, 595, 596, 597)


def _fp8(shape, dev, gen):
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)
    x[(x & 0x7F) == 0x7F] = 0x7E   # no NaN codes
    return x.view(torch.float8_e4m3fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    args = ap.parse_args()
    import qutlass_amd as q
    from qutlass_amd.utils import to_blocked

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_mxf8_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_int, ctypes.c_void_p]
    fp = q._lib.load().qutlass_amd_debug_grouped_mxf8_plan
    fp.restype = ctypes.c_int
    fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'grouped_us':>10s} {'loop_us':>9s} {'x':>6s} {'TB/s':>6s}"
    if args.forms:
        hdr += "  " + " ".join(f"{v:>7d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    for model, proj, E, N, K, topk in LAYERS:
        b = _fp8((E, N, K), dev, gen)
        b_sf = torch.randint(124, 131, (E * N * K // 32,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        kb = K // 32
        b_blk = [to_blocked(b_sf[g * N * kb:(g + 1) * N * kb].view(N, kb)) for g in range(E)]
        for phase, T in TOKENS.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            a = _fp8((M, K), dev, gen)
            a_sf = torch.randint(124, 131, (M * K // 32,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
            alpha = torch.ones(1, device=dev)
            for kind in ("uniform", "skewed"):
                if args.quick and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                ends = np.cumsum(c)
                offs = torch.tensor(ends, dtype=torch.int32, device=dev)
                o = [0] + ends.tolist()
                live = [g for g in range(E) if c[g] > 0]
                # the loop's blocked scales, one to_blocked per group (128-row padding): prepared here, outside the timed region
                views = [(a[o[g]:o[g + 1]], b[g], to_blocked(a_sf[o[g] * kb:o[g + 1] * kb].view(o[g + 1] - o[g], kb)), b_blk[g]) for g in live]

                def grouped():
                    q.grouped_matmul_mxf8_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

                def loop():
                    for av, bv, asv, bsv in views:
                        q.matmul_mxf8_bf16_tn(av, bv, asv, bsv, alpha)

                tg = bench_graph(grouped, args.reps)[0] * 1e3
                tl = bench_graph(loop, args.reps)[0] * 1e3
                wbytes = len(live) * N * (K + K // 32)
                form = str(fp(M, N, K, E, None))
                line = f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {tg:10.2f} {tl:9.2f} {tl / tg:6.2f} {wbytes / tg / 1e6:6.2f}"
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, grouped_us=round(tg, 3), loop_us=round(tl, 3),
                           weight_TBps=round(wbytes / tg / 1e6, 3))
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    ft = {}
                    for v in FORMS:
                        def forced():
                            f(a.data_ptr(), b.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), out.data_ptr(), M, N, K, E, 0,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                    line += "  " + " ".join(f"{ft[v]:7.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(t, 3) for v, t in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
                del views
            del a, a_sf
        del b, b_sf, b_blk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
