#!/usr/bin/env python3
"""Grouped MXFP4 GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf4_bf16_tn) against the loop it replaces: one matmul_ada_mxf4_bf16_tn per
expert with the group offsets already on the host (the loop's best case -- a real caller pays a device -> host sync for them and cannot capture the loop).

    grouped_us   one launch over all experts (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays)
    loop_us      E launches of matmul_ada_mxf4_bf16_tn, one per non-empty group, captured into the same kind of graph
    TB/s         bytes of the weights of the non-empty groups (e2m1 + e8m0) / grouped time
    --forms      also every form of the grouped op forced through the lab library (590 = 32x32, 591 = 32x16, 592 = 64x32, 593 = 64x64 ring): the calibration
                 of the form rule (qutlass_amd/csrc/capi.hip grouped_plan)

Shapes: Qwen3-30B-A3B (E = 128, top-8) and Mixtral-8x7B (E = 8, top-2) gate/up and down projections at decode (64 tokens) and prefill (4096 tokens), uniform and
skewed routing (half of the routed rows in one expert).  Operands are random codes with scale bytes near 127 (timing only).

    python benchmarks/bench_grouped_mxfp4_mi355x.py [--reps 50] [--forms] [--quick]
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

_spec = importlib.util.spec_from_file_location("bench_mxfp4_mi355x", os.path.join(ROOT, "benchmarks", "bench_mxfp4_mi355x.py"))
_bm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_bm)
bench_graph = _bm.bench_graph

# (model, projection, E, N, K, top-k)
LAYERS = [
    ("Qwen3-30B-A3B", "gate_up", 128, 1536, 2048, 8),
    ("Qwen3-30B-A3B", "down", 128, 2048, 768, 8),
    ("Mixtral-8x7B", "gate_up", 8, 28672, 4096, 2),
    ("Mixtral-8x7B", "down", 8, 4096, 14336, 2),
]
TOKENS = {"decode": 64, "prefill": 4096}


def routing(M, E, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        c = np.bincount(rng.integers(0, E, M), minlength=E)
    else:   # skewed: half of the rows in one expert
        c = np.bincount(rng.integers(0, E, M - M // 2), minlength=E)
        c[0] += M // 2
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_mxf4_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'grouped_us':>10s} {'loop_us':>9s} {'x':>6s} {'TB/s':>6s}"
    if args.forms:
        hdr += "  " + " ".join(f"{v:>7d}" for v in (590, 591, 592, 593))
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    for model, proj, E, N, K, topk in LAYERS:
        b = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = torch.randint(124, 131, (E * N * K // 32,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        for phase, T in TOKENS.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            a = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=gen)
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
                kb = K // 32
                views = [(a[o[g]:o[g + 1]], b[g], a_sf[o[g] * kb:o[g + 1] * kb], b_sf[g * N * kb:(g + 1) * N * kb]) for g in live]

                def grouped():
                    q.grouped_matmul_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

                def loop():
                    for av, bv, asv, bsv in views:
                        q.matmul_ada_mxf4_bf16_tn(av, bv, asv, bsv, alpha)

                tg = bench_graph(grouped, args.reps)[0] * 1e3
                tl = bench_graph(loop, args.reps)[0] * 1e3
                wbytes = len(live) * N * (K // 2 + K // 32)
                plan = q._lib.load()
                form = ""
                try:
                    fp = plan.qutlass_amd_debug_grouped_plan
                    fp.restype = ctypes.c_int
                    fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
                    form = str(fp(M, N, K, E, None))
                except AttributeError:
                    pass
                line = f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {tg:10.2f} {tl:9.2f} {tl / tg:6.2f} {wbytes / tg / 1e6:6.2f}"
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, grouped_us=round(tg, 3), loop_us=round(tl, 3),
                           weight_TBps=round(wbytes / tg / 1e6, 3))
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    ft = {}
                    for v in (590, 591, 592, 593):
                        def forced():
                            f(a.data_ptr(), b.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), out.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                    line += "  " + " ".join(f"{ft[v]:7.2f}" for v in (590, 591, 592, 593))
                    rec["forms_us"] = {str(v): round(t, 3) for v, t in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del a, a_sf
        del b, b_sf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
