#!/usr/bin/env python3
"""W4A16 grouped GEMM of mixture-of-experts layers (qutlass_amd.grouped_matmul_bf16_mxf4_bf16_tn: bf16 tokens against MXFP4 expert weights) against what a caller
runs without it, on the same tokens, expert weights and routing:

    w4a16_us     the op on sorted tokens, the form its rule picks (graph-timed like benchmarks/bench_mxfp4_mi355x.py: median of HIP-graph replays; q20 / q80 beside it)
    w4a16_2_us   the same measurement taken a second time after the other columns: the run-to-run spread of this table
    (a) w4a8_us  grouped_matmul_mxf8_mxf4_bf16_tn alone on e4m3 tokens -- the same weight bytes, 8-bit token numerics; xa = w4a8_us / w4a16_us
    (b) gate/up only, from the UNSORTED tokens and src_row:
        gath_us  this op with src_row (the gather in the GEMM)
        sel_us   x.index_select(0, src_row) + this op: what the gather replaces on this path; xs = sel_us / gath_us
        q8_us    fusedGatherQuantizeMxf8 + the W4A8 op: the chain this op replaces; xq = q8_us / gath_us
    (c) bf16_us  one torch bf16 matmul per non-empty expert on weights dequantised to bf16 (four times the weight bytes; the group sizes known on the host, the
                 loop's best case); xc = bf16_us / w4a16_us
    every x: above 1 this op is faster
    --forms      also every form of the op forced through the lab library (606 = 32x32, 607 = 32x16, 608 = 64x32): the calibration of the form rule
                 (qutlass_amd/csrc/capi.hip grouped_w4a16_plan)

Shapes: the decode (64 tokens) and prefill (4096 tokens) gate/up and down projections of Qwen3-30B-A3B, Mixtral-8x7B, gpt-oss-20b and gpt-oss-120b
(benchmarks/bench_grouped_w4a8_mi355x.py), uniform and skewed routing.  Operands are random (timing only): Gaussian tokens, random codes, scale bytes near 127.

    --sweep      instead of the models: 128 experts, N = 2048, a mean of 16 ... 128 rows per expert at K = 512 ... 2944 -- where the rule's two thresholds lie

    python benchmarks/bench_grouped_w4a16_mi355x.py [--reps 50] [--forms] [--quick] [--only SUBSTRING] [--sweep] [--no-bf16]
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

FORMS = (606, 607, 608)
SWEEP_ROWS, SWEEP_K = (16, 32, 48, 64, 128), (512, 768, 1024, 1152, 1536, 2048, 2944)
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def _dequant_bf16(b4, b_sf):
    """(E, N, K/2) packed e2m1, (E N K/32) e8m0 -> (E, N, K) bf16, expert by expert"""
    lut = torch.tensor(E2M1, dtype=torch.bfloat16, device=b4.device)
    E, N, K2 = b4.shape
    sf = torch.exp2(b_sf.view(torch.uint8).view(E, N, K2 // 16).float() - 127.0).to(torch.bfloat16)
    out = torch.empty(E, N, 2 * K2, dtype=torch.bfloat16, device=b4.device)
    for g in range(E):
        out[g, :, 0::2] = lut[(b4[g] & 0xF).long()]
        out[g, :, 1::2] = lut[(b4[g] >> 4).long()]
        out[g] = (out[g].view(N, K2 // 16, 32) * sf[g][:, :, None]).view(N, 2 * K2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time every form forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--sweep", action="store_true", help="rows per expert x K around the form rule's thresholds instead of the models")
    ap.add_argument("--no-bf16", action="store_true", help="without column (c)")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn
        f.restype = ctypes.c_int
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        f.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp]
    plans = {}
    for name in ("bf16_mxf4", "mxf8_mxf4"):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_grouped_{name}_plan")
        fp.restype = ctypes.c_int
        fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = (f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'w4a16_us':>9s} {'q20':>8s} {'q80':>8s} {'w4a16_2_us':>10s} "
           f"{'f8':>4s} {'w4a8_us':>9s} {'xa':>5s} {'gath_us':>9s} {'sel_us':>9s} {'xs':>5s} {'q8_us':>9s} {'xq':>5s} {'bf16_us':>9s} {'xc':>5s} {'TB/s':>6s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    eye = torch.eye(32, dtype=torch.bfloat16, device=dev)
    layers = [("sweep", f"K{K}", 128, 2048, K, 1) for K in SWEEP_K] if args.sweep else LAYERS
    tokens = {f"r{r}": 128 * r for r in SWEEP_ROWS} if args.sweep else TOKENS
    nan = float("nan")
    for model, proj, E, N, K, topk in layers:
        if args.only and args.only not in model:
            continue
        kb = K // 32
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = torch.randint(124, 131, (E * N * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        wbf = None if (args.no_bf16 or args.sweep) else _dequant_bf16(b4, b_sf)
        for phase, T in tokens.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            x = torch.randn(T, K, dtype=torch.bfloat16, device=dev, generator=gen)          # the unsorted tokens
            a8 = _fp8((M, K), dev, gen)
            a_sf = torch.randint(124, 131, (M * kb,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
            alpha = torch.ones(1, device=dev)
            for kind in ("uniform", "skewed"):
                if (args.quick or args.sweep) and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)
                ends = np.concatenate([[0], np.cumsum(c)])
                live = int((c > 0).sum())
                src_row = torch.from_numpy(np.random.default_rng(1).permutation(M).astype(np.int32) // topk).to(dev)   # every token in top-k groups
                src_long = src_row.long()
                a16 = x.index_select(0, src_long)                                                # the sorted tokens

                def w4a16():
                    q.grouped_matmul_bf16_mxf4_bf16_tn(a16, b4, b_sf, alpha, offs)

                def w4a8():
                    q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b4, a_sf, b_sf, alpha, offs)

                def gath():
                    q.grouped_matmul_bf16_mxf4_bf16_tn(x, b4, b_sf, alpha, offs, src_row=src_row)

                def sel():
                    q.grouped_matmul_bf16_mxf4_bf16_tn(x.index_select(0, src_long), b4, b_sf, alpha, offs)

                def q8():
                    aq, asf = q.fusedGatherQuantizeMxf8(x, eye, src_row)
                    q.grouped_matmul_mxf8_mxf4_bf16_tn(aq, b4, asf, b_sf, alpha, offs)

                def bf16():
                    for g in range(E):
                        if c[g]:
                            torch.matmul(a16[ends[g]:ends[g + 1]], wbf[g].t())

                t, lo, hi = (v * 1e3 for v in bench_graph(w4a16, args.reps)[:3])
                t8 = bench_graph(w4a8, args.reps)[0] * 1e3
                tg = ts = tq = nan
                if proj == "gate_up":
                    tg, ts, tq = (bench_graph(fn, args.reps)[0] * 1e3 for fn in (gath, sel, q8))
                tc = nan
                if wbf is not None:
                    try:
                        tc = bench_graph(bf16, args.reps)[0] * 1e3
                    except RuntimeError as e:   # a BLAS that cannot be captured: the column stays empty
                        print(f"# bf16 matmul loop not timed: {str(e).splitlines()[0]}")
                        torch.cuda.synchronize()
                ft = {}
                if args.forms:
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                    for v in FORMS:
                        def forced():
                            f(a16.data_ptr(), b4.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), None, 0, out.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(w4a16, args.reps)[0] * 1e3
                wbytes = live * N * (K // 2 + kb)
                form, f8 = (str(plans[n](M, N, K, E, None)) for n in ("bf16_mxf4", "mxf8_mxf4"))
                line = (f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {t2:10.2f} {f8:>4s} {t8:9.2f} {t8 / t:5.2f} "
                        f"{tg:9.2f} {ts:9.2f} {ts / tg:5.2f} {tq:9.2f} {tq / tg:5.2f} {tc:9.2f} {tc / t:5.2f} {wbytes / t / 1e6:6.2f}")
                r3 = lambda v: None if v != v else round(v, 3)
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, w4a16_us=r3(t), w4a16_q20_us=r3(lo), w4a16_q80_us=r3(hi),
                           w4a16_again_us=r3(t2), w4a8_form=f8, w4a8_us=r3(t8), gather_us=r3(tg), index_select_us=r3(ts), gather_quantize_w4a8_us=r3(tq), bf16_loop_us=r3(tc),
                           weight_TBps=r3(wbytes / t / 1e6))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(v2, 3) for v, v2 in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del x, a8, a_sf
        del b4, b_sf, wbf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
