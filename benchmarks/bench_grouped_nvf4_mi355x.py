#!/usr/bin/env python3
"""Grouped NVFP4 GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_nvf4_bf16_tn) against the loop it replaces: one matmul_nvf4_bf16_tn per
expert with the group offsets already on the host and every group's to_blocked scales prepared outside the timed region (the loop's best case -- a real
caller pays a device -> host sync for the offsets, one to_blocked per group, and cannot capture the loop).

    grouped_us   one launch over all experts (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays)
    loop_us      E launches of matmul_nvf4_bf16_tn, one per non-empty group, captured into the same kind of graph
    TB/s         bytes of the weights of the non-empty groups (e2m1 + e4m3 scales) / grouped time
    --forms      also every form of the grouped op forced through the lab library (598 = 32x32, 599 = 64x32 tiles of the wave-owned kernel, 600 = 64x64, 601 = 128x128 tiles of the
                 tile kernel): the calibration of the form rule (qutlass_amd/csrc/capi.hip grouped_nv_plan)
    spread       (max - min) / median of the grouped time over --repeat whole measurements of the row (the run-to-run spread of the session)

Shapes, routings and timing: those of benchmarks/bench_grouped_mxfp4_mi355x.py (Qwen3-30B-A3B and Mixtral-8x7B gate/up and down projections at decode and
prefill, uniform and skewed routing).  Operands are random e2m1 codes with e4m3 scale bytes 0x30 ... 0x47 (timing only).

    python benchmarks/bench_grouped_nvf4_mi355x.py [--reps 50] [--repeat 3] [--forms] [--quick]
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

FORMS = (598, 599, 600, 601)


def _fp4(shape, dev, gen):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)


def _sf(n, dev, gen):
    return torch.randint(0x30, 0x48, (n,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e4m3fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (grouped and loop alternate); the medians are reported, the spread is the grouped op's")
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--tokens", default="", help="calibration: comma-separated token counts instead of decode (64) and prefill (4096)")
    ap.add_argument("--edges", action="store_true", help="calibration: also the Mixtral down projection cut to K = 6144 and 8192 (where the small-batch forms cross)")
    args = ap.parse_args()
    import qutlass_amd as q
    from qutlass_amd.utils import to_blocked

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_nvf4_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    fp = q._lib.load().qutlass_amd_debug_grouped_nvf4_plan
    fp.restype = ctypes.c_int
    fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = f"{'model':14s} {'proj':10s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'grouped_us':>10s} {'loop_us':>9s} {'x':>6s} {'TB/s':>6s} {'spread':>6s}"
    if args.forms:
        hdr += "  " + " ".join(f"{v:>7d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    tokens = {f"t{t}": int(t) for t in args.tokens.split(",")} if args.tokens else TOKENS
    layers = LAYERS + ([("Mixtral-8x7B", "down/K6144", 8, 4096, 6144, 2), ("Mixtral-8x7B", "down/K8192", 8, 4096, 8192, 2)] if args.edges else [])
    for model, proj, E, N, K, topk in layers:
        b = _fp4((E, N, K // 2), dev, gen)
        b_sf = _sf(E * N * K // 16, dev, gen)
        kb = K // 16
        b_blk = [to_blocked(b_sf[g * N * kb:(g + 1) * N * kb].view(N, kb)) for g in range(E)]
        for phase, T in tokens.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            a = _fp4((M, K // 2), dev, gen)
            a_sf = _sf(M * K // 16, dev, gen)
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
                    q.grouped_matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

                def loop():
                    for av, bv, asv, bsv in views:
                        q.matmul_nvf4_bf16_tn(av, bv, asv, bsv, alpha)

                tgs, tls = [], []
                for _ in range(max(1, args.repeat)):
                    tgs.append(bench_graph(grouped, args.reps)[0] * 1e3)
                    tls.append(bench_graph(loop, args.reps)[0] * 1e3)
                tg, tl = float(np.median(tgs)), float(np.median(tls))
                spread = (max(tgs) - min(tgs)) / tg
                wbytes = len(live) * N * (K // 2 + K // 16)
                form = str(fp(M, N, K, E, None))
                line = f"{model:14s} {proj:10s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {tg:10.2f} {tl:9.2f} {tl / tg:6.2f} {wbytes / tg / 1e6:6.2f} {spread:6.3f}"
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, grouped_us=round(tg, 3), loop_us=round(tl, 3),
                           weight_TBps=round(wbytes / tg / 1e6, 3), spread=round(spread, 4), loop_spread=round((max(tls) - min(tls)) / tl, 4))
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    ft = {}
                    for v in FORMS:
                        def forced():
                            f(a.data_ptr(), b.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), out.data_ptr(), M, N, K, E,
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
