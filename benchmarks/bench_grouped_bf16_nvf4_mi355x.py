#!/usr/bin/env python3
"""W4A16 grouped GEMM on NVFP4 expert weights (qutlass_amd.grouped_matmul_bf16_nvf4_bf16_tn: bf16 tokens against e2m1 codes with e4m3 group scales) against what a
caller runs without it, on the same tokens, routing and weight codes (graph-timed like benchmarks/bench_grouped_w4a16_mi355x.py: median of HIP-graph replays):

    nv16_us      the op on sorted tokens, the form its rule picks; q20 / q80 beside it
    nv16_2_us    the same measurement taken a second time after the other columns: the run-to-run spread of this table
    (a) mx16_us  grouped_matmul_bf16_mxf4_bf16_tn on MXFP4 weights of the same shape (the same codes, e8m0 scales): weights through LDS and one convert per two
                 elements, against weights in registers and three; xa = mx16_us / nv16_us
    (b) gate/up only, from the UNSORTED tokens and src_row:
        gath_us  this op with src_row (the gather in the GEMM)
        sel_us   x.index_select(0, src_row) + this op; xs = sel_us / gath_us
        q4_us    fusedGatherQuantizeNvGrouped + grouped_matmul_nvf4_bf16_tn: the W4A4 chain this op is the alternative to; xq = q4_us / gath_us
    (c) bf16_us  one torch bf16 matmul per non-empty expert on weights dequantised to bf16 (group sizes known on the host, the loop's best case); xc = bf16_us / nv16_us
    every x: above 1 this op is faster
    --forms      also both forms forced through the lab library (620 = 32x32, 621 = 64x32): the calibration of qutlass_amd/csrc/capi.hip grouped_bf16_nvf4_plan

Shapes: the decode (64 tokens) and prefill (4096 tokens) gate/up and down projections of Qwen3-30B-A3B, Mixtral-8x7B, gpt-oss-20b and gpt-oss-120b, uniform and
skewed routing.  Operands are random (timing only): Gaussian tokens, random codes, finite scale bytes.

    python benchmarks/bench_grouped_bf16_nvf4_mi355x.py [--reps 50] [--forms] [--quick] [--only SUBSTRING] [--no-bf16] [--accuracy]
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

FORMS = (620, 621)
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def _dequant_bf16(b4, b_sf):
    """(E, N, K/2) packed e2m1, (E N K/16) e4m3 -> (E, N, K) bf16, expert by expert"""
    lut = torch.tensor(E2M1, dtype=torch.bfloat16, device=b4.device)
    E, N, K2 = b4.shape
    sf = b_sf.view(E, N, K2 // 8).to(torch.bfloat16)
    out = torch.empty(E, N, 2 * K2, dtype=torch.bfloat16, device=b4.device)
    for g in range(E):
        out[g, :, 0::2] = lut[(b4[g] & 0xF).long()]
        out[g, :, 1::2] = lut[(b4[g] >> 4).long()]
        out[g] = (out[g].view(N, K2 // 8, 16) * sf[g][:, :, None]).view(N, 2 * K2)
    return out


def accuracy(q, dev):
    """--accuracy: a 64-token gated layer (8 experts, top-2, H = I = 256) on NVFP4 weights, |L - L_fp64| / |L_fp64| with L_fp64 fp64 mathematics
    on the dequantised weights -- this op on bf16 tokens beside the W4A4 chain (gathering and gated NVFP4 quantizers + grouped_matmul_nvf4_bf16_tn) on the same bytes"""
    T, E, H, I = 64, 8, 256, 256
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    tok, eye, gs, ags = rn(T, H).bfloat16(), torch.eye(32, dtype=torch.bfloat16, device=dev), torch.full((E,), 6.0, device=dev), torch.full((E,), 4.0, device=dev)
    weights, ids, src_row, offs, pos = q.moe_route(rn(T, E), 2)
    wts = []
    for N, K in ((2 * I, H), (H, I)):   # the checkpoint's bytes: the library's abs-max NVFP4 quantizer without a rotation, weight global scale 6
        c, s = q.fusedQuantizeNv((0.2 * rn(E * N, K)).bfloat16(), eye, gs[:1])
        wts.append((c.view(E, N, K // 2), s.view(torch.uint8).view(-1)[:E * N * K // 16].clone().view(torch.float8_e4m3fn)))
    (w13, s13), (w2, s2) = wts
    a16, a4 = 1.0 / gs, 1.0 / (gs * ags)
    y16 = q.grouped_matmul_bf16_nvf4_bf16_tn(q.silu_and_mul(q.grouped_matmul_bf16_nvf4_bf16_tn(tok, w13, s13, a16, offs, src_row=src_row)), w2, s2, a16, offs)
    aq, asf = q.fusedGatherQuantizeNvGrouped(tok, eye, ags, src_row, offs)
    bq, bsf = q.fusedSiluMulQuantizeNvGrouped(q.grouped_matmul_nvf4_bf16_tn(aq, w13, asf, s13, a4, offs), eye, ags, offs)
    y4 = q.grouped_matmul_nvf4_bf16_tn(bq, w2, bsf, s2, a4, offs)
    l16, l4 = (q.moe_combine(y, pos, weights).double().cpu().numpy() for y in (y16, y4))

    def deq(c, s):   # (E, N, K/2) packed e2m1, flat e4m3 scales -> the fp64 weights (E, N, K), the global scale 6 taken out
        c = c.cpu().numpy()
        codes = np.stack([c & 0xF, c >> 4], axis=-1).reshape(*c.shape[:2], -1)
        return np.array(E2M1)[codes] * np.repeat(s.float().cpu().numpy().astype(np.float64), 16).reshape(codes.shape) / 6.0

    d13, d2, xs, ends = deq(w13, s13), deq(w2, s2), tok.double().cpu().numpy()[src_row.cpu().numpy()], np.concatenate([[0], offs.cpu().numpy()])
    y64 = np.zeros((2 * T, H))
    for e in range(E):
        gu = xs[ends[e]:ends[e + 1]] @ d13[e].T
        y64[ends[e]:ends[e + 1]] = (gu[:, :I] / (1.0 + np.exp(-gu[:, :I])) * gu[:, I:]) @ d2[e].T
    l64 = (weights.double().cpu().numpy()[:, :, None] * y64[pos.cpu().numpy()]).sum(axis=1)
    e16, e4 = (float(np.linalg.norm(l - l64) / np.linalg.norm(l64)) for l in (l16, l4))
    assert np.isfinite(l16).all() and np.isfinite(l4).all()
    print(f"# 64-token gated layer on NVFP4 weights (E 8, top-2, H = I = 256), |L_gpu - L_fp64| / |L_fp64|: W4A16 (this op) {e16:.5f}, W4A4 chain {e4:.5f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time both forms forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--no-bf16", action="store_true", help="without column (c)")
    ap.add_argument("--accuracy", action="store_true", help="instead of the timings: the layer's error against fp64 beside the W4A4 chain's")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    if args.accuracy:
        return accuracy(q, dev)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_bf16_nvf4_bf16_tn
        f.restype, f.argtypes = ctypes.c_int, [vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp]
    plans = {}
    for name in ("bf16_nvf4", "bf16_mxf4", "nvf4"):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_grouped_{name}_plan")
        fp.restype, fp.argtypes = ctypes.c_int, [i64] * 4 + [vp]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}")
    hdr = (f"{'model':14s} {'proj':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'N':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'nv16_us':>9s} {'q20':>8s} {'q80':>8s} {'nv16_2_us':>10s} "
           f"{'fmx':>4s} {'mx16_us':>9s} {'xa':>5s} {'gath_us':>9s} {'sel_us':>9s} {'xs':>5s} {'f4':>4s} {'q4_us':>9s} {'xq':>5s} {'bf16_us':>9s} {'xc':>5s} {'TB/s':>6s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    eye = torch.eye(32, dtype=torch.bfloat16, device=dev)
    nan = float("nan")
    for model, proj, E, N, K, topk in LAYERS:
        if args.only and args.only not in model:
            continue
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = _fp8((E * N * K // 16,), dev, gen)                                                  # any finite e4m3 byte
        b_sf8 = torch.randint(124, 131, (E * N * K // 32,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e8m0fnu)
        wbf = None if args.no_bf16 else _dequant_bf16(b4, b_sf)
        for phase, T in TOKENS.items():
            if args.quick and phase != "decode":
                continue
            M = T * topk
            x = torch.randn(T, K, dtype=torch.bfloat16, device=dev, generator=gen)          # the unsorted tokens
            alpha, gs = torch.ones(E, device=dev), torch.ones(E, device=dev)
            for kind in ("uniform", "skewed"):
                if args.quick and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)
                ends = np.concatenate([[0], np.cumsum(c)])
                live = int((c > 0).sum())
                src_row = torch.from_numpy(np.random.default_rng(1).permutation(M).astype(np.int32) // topk).to(dev)   # every token in top-k groups
                src_long = src_row.long()
                a16 = x.index_select(0, src_long)                                                # the sorted tokens

                def nv16():
                    q.grouped_matmul_bf16_nvf4_bf16_tn(a16, b4, b_sf, alpha, offs)

                def mx16():
                    q.grouped_matmul_bf16_mxf4_bf16_tn(a16, b4, b_sf8, alpha, offs)

                def gath():
                    q.grouped_matmul_bf16_nvf4_bf16_tn(x, b4, b_sf, alpha, offs, src_row=src_row)

                def sel():
                    q.grouped_matmul_bf16_nvf4_bf16_tn(x.index_select(0, src_long), b4, b_sf, alpha, offs)

                def q4():
                    aq, asf = q.fusedGatherQuantizeNvGrouped(x, eye, gs, src_row, offs)
                    q.grouped_matmul_nvf4_bf16_tn(aq, b4, asf, b_sf, alpha, offs)

                def bf16():
                    for g in range(E):
                        if c[g]:
                            torch.matmul(a16[ends[g]:ends[g + 1]], wbf[g].t())

                t, lo, hi = (v * 1e3 for v in bench_graph(nv16, args.reps)[:3])
                tm = bench_graph(mx16, args.reps)[0] * 1e3
                tg = ts = tq = nan
                if proj == "gate_up":
                    tg, ts, tq = (bench_graph(fn, args.reps)[0] * 1e3 for fn in (gath, sel, q4))
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
                            f(a16.data_ptr(), b4.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), E, offs.data_ptr(), None, 0, out.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(nv16, args.reps)[0] * 1e3
                wbytes = live * N * (K // 2 + K // 16)
                form, fmx, f4 = (str(plans[n](M, N, K, E, None)) for n in ("bf16_nvf4", "bf16_mxf4", "nvf4"))
                line = (f"{model:14s} {proj:8s} {phase:8s} {kind:8s} {E:4d} {N:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {t2:10.2f} {fmx:>4s} {tm:9.2f} {tm / t:5.2f} "
                        f"{tg:9.2f} {ts:9.2f} {ts / tg:5.2f} {f4:>4s} {tq:9.2f} {tq / tg:5.2f} {tc:9.2f} {tc / t:5.2f} {wbytes / t / 1e6:6.2f}")
                r3 = lambda v: None if v != v else round(v, 3)
                rec = dict(model=model, proj=proj, phase=phase, routing=kind, E=E, N=N, K=K, M=M, form=form, nv16_us=r3(t), nv16_q20_us=r3(lo), nv16_q80_us=r3(hi),
                           nv16_again_us=r3(t2), mx16_form=fmx, mx16_us=r3(tm), gather_us=r3(tg), index_select_us=r3(ts), w4a4_form=f4, gather_quantize_w4a4_us=r3(tq),
                           bf16_loop_us=r3(tc), weight_TBps=r3(wbytes / t / 1e6))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(v2, 3) for v, v2 in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del x
        del b4, b_sf, b_sf8, wbf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
