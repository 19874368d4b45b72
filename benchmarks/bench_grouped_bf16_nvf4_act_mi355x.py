#!/usr/bin/env python3
"""The gate/up W4A16 grouped GEMM on NVFP4 weights with fused activation (qutlass_amd.grouped_matmul_bf16_nvf4_silu_bf16_tn / ..._swiglu_oai_bf16_tn) against the two
launches it replaces, on the same tokens, expert weights and routing (graph-timed like benchmarks/bench_grouped_w4a16_act_mi355x.py: median of HIP-graph replays; the
two sides alternate in one process and each is taken twice):

    act_us       (a) the fused op, the form its rule picks; q20 / q80 beside it
    chain_us     (b) grouped_matmul_bf16_nvf4_bf16_tn, then swiglu_oai_and_mul (with bias) / silu_and_mul on its output
    gemm_us      (c) grouped_matmul_bf16_nvf4_bf16_tn alone: chain_us - gemm_us is the saved launch, gemm_us - act_us what the tile gains or loses
    act_2_us, chain_2_us   (a) and (b) a second time, after the other columns; spread = the larger of |take 2 / take 1 - 1| of the two: the run-to-run spread of the cell
    b/a, c/a     chain_us / act_us and gemm_us / act_us from the first takes: above 1 the fused op is faster; a b/a below 1 - spread is printed between ** **
    --forms      also both forms forced through the lab library (622 = 32 rows x 32 activation columns, 623 = 64 x 32): the calibration of the form rule
                 (qutlass_amd/csrc/capi.hip grouped_bf16_nvf4_act_plan)
    --gather     the tokens stay unsorted and both (a) and (b) read them through src_row

Cells: the gate/up projections of gpt-oss-20b / 120b (clamped SwiGLU with bias; I = H = 2944, 2880 padded to K % 128 == 0), Qwen3-30B-A3B and Mixtral-8x7B (silu), at
16 and 64 tokens (decode) and 4096 (prefill), uniform and skewed routing.  Operands are Gaussian bf16 tokens, random weight codes and e4m3 scale bytes near 1 (timing only).

    --sweep      instead of the models: 128 experts, I = 1024, silu, a mean of 16 ... 128 rows per expert at K = 512 ... 2944 -- where the rule's thresholds lie
    --accuracy   instead of the timings: a 64-token gated layer through the fused op and through the three launches, each against fp64 mathematics

    python benchmarks/bench_grouped_bf16_nvf4_act_mi355x.py [--reps 50] [--forms] [--gather] [--quick] [--only SUBSTRING] [--sweep] [--accuracy]
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
bench_graph, routing = _g4.bench_graph, _g4.routing

LAYERS = [   # model, activation, E, I, K, top-k
    ("gpt-oss-20b", "oai_bias", 32, 2944, 2944, 4),
    ("gpt-oss-120b", "oai_bias", 128, 2944, 2944, 4),
    ("Qwen3-30B-A3B", "silu", 128, 768, 2048, 8),
    ("Mixtral-8x7B", "silu", 8, 14336, 4096, 2),
]
TOKENS = {"decode16": 16, "decode64": 64, "prefill": 4096}
FORMS = (622, 623)
SWEEP_ROWS, SWEEP_K = (16, 32, 48, 64, 128), (512, 768, 1024, 1280, 2048, 2944)
ACT_ALPHA, LIMIT = 1.702, 7.0
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def accuracy(q, dev):
    """--accuracy: the 64-token gated layer of bench_grouped_bf16_nvf4_mi355x.py --accuracy (8 experts, top-2, H = I = 256, NVFP4 weights),
    |L - L_fp64| / |L_fp64| with L_fp64 fp64 mathematics on the dequantised weights -- the fused op + down GEMM beside the three launches; the bits are equal, so the
    errors are"""
    T, E, H, I = 64, 8, 256, 256
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    tok, eye, gs = rn(T, H).bfloat16(), torch.eye(32, dtype=torch.bfloat16, device=dev), torch.full((E,), 6.0, device=dev)
    weights, ids, src_row, offs, pos = q.moe_route(rn(T, E), 2)
    wts = []
    for N, K in ((2 * I, H), (H, I)):   # the checkpoint's bytes: the library's abs-max NVFP4 quantizer without a rotation, weight global scale 6
        c, s = q.fusedQuantizeNv((0.2 * rn(E * N, K)).bfloat16(), eye, gs[:1])
        wts.append((c.view(E, N, K // 2), s.view(torch.uint8).view(-1)[:E * N * K // 16].clone().view(torch.float8_e4m3fn)))
    (w13, s13), (w2, s2) = wts
    a16 = 1.0 / gs
    h3 = q.silu_and_mul(q.grouped_matmul_bf16_nvf4_bf16_tn(tok, w13, s13, a16, offs, src_row=src_row))
    h1 = q.grouped_matmul_bf16_nvf4_silu_bf16_tn(tok, w13, s13, a16, offs, src_row=src_row)
    l3, l1 = (q.moe_combine(q.grouped_matmul_bf16_nvf4_bf16_tn(h, w2, s2, a16, offs), pos, weights).double().cpu().numpy() for h in (h3, h1))

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
    e3, e1 = (float(np.linalg.norm(l - l64) / np.linalg.norm(l64)) for l in (l3, l1))
    assert np.isfinite(l3).all() and np.isfinite(l1).all()
    print(f"# 64-token gated layer on NVFP4 weights (E 8, top-2, H = I = 256), |L_gpu - L_fp64| / |L_fp64|: fused gate/up + down (two launches) {e1:.5f}, "
          f"gate/up + silu_and_mul + down (three launches) {e3:.5f}; hidden activations bit-equal: {bool(torch.equal(h1.view(torch.int16), h3.view(torch.int16)))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time both forms forced through the lab library")
    ap.add_argument("--gather", action="store_true", help="unsorted tokens read through src_row")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--sweep", action="store_true", help="rows per expert x K around the form rule's thresholds instead of the models")
    ap.add_argument("--accuracy", action="store_true", help="instead of the timings: the layer's error against fp64 through the fused op and through the three launches")
    args = ap.parse_args()
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    if args.accuracy:
        return accuracy(q, dev)
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_bf16_nvf4_act_bf16_tn
        f.restype = ctypes.c_int
        f.argtypes = ([ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 2
                      + [ctypes.c_int64] * 4 + [ctypes.c_void_p])
    plans = {}
    for name in ("bf16_nvf4_act", "bf16_nvf4"):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_grouped_{name}_plan")
        fp.restype = ctypes.c_int
        fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}  gather={int(args.gather)}")
    hdr = (f"{'model':14s} {'act':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'I':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'act_us':>9s} {'q20':>8s} {'q80':>8s} {'fg':>4s} "
           f"{'chain_us':>9s} {'gemm_us':>9s} {'act_2_us':>9s} {'chain_2_us':>10s} {'spread':>6s} {'b/a':>8s} {'c/a':>6s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    layers = [("sweep", "silu", 128, 1024, K, 1) for K in SWEEP_K] if args.sweep else LAYERS
    tokens = {f"r{r}": 128 * r for r in SWEEP_ROWS} if args.sweep else TOKENS
    for model, act, E, inter, K, topk in layers:
        if args.only and args.only not in model:
            continue
        ks, N = K // 16, 2 * inter
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = torch.randint(0x30, 0x40, (E * N * ks,), dtype=torch.uint8, device=dev, generator=gen).view(torch.float8_e4m3fn)   # 0.5 ... 1.875
        bias = torch.randn(E, N, device=dev, generator=gen).to(torch.bfloat16) if act == "oai_bias" else None
        for phase, T in tokens.items():
            if args.quick and not phase.startswith("decode"):
                continue
            M = T * topk
            x = torch.randn(T if args.gather else M, K, device=dev, generator=gen).to(torch.bfloat16)
            src = (torch.randperm(M, device=dev, generator=gen) % T).to(torch.int32) if args.gather else None
            alpha = torch.full((1,), 2.0 ** -6, device=dev)
            for kind in ("uniform", "skewed"):
                if (args.quick or args.sweep) and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)

                def gemm():
                    return q.grouped_matmul_bf16_nvf4_bf16_tn(x, b4, b_sf, alpha, offs, src_row=src)

                if act == "silu":
                    def fused():
                        q.grouped_matmul_bf16_nvf4_silu_bf16_tn(x, b4, b_sf, alpha, offs, src_row=src)

                    def chain():
                        q.silu_and_mul(gemm())
                else:
                    def fused():
                        q.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn(x, b4, b_sf, alpha, offs, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias, src_row=src)

                    def chain():
                        q.swiglu_oai_and_mul(gemm(), alpha=ACT_ALPHA, limit=LIMIT, bias=bias, offs=offs)

                t, lo, hi = (v * 1e3 for v in bench_graph(fused, args.reps)[:3])
                tb = bench_graph(chain, args.reps)[0] * 1e3
                tc = bench_graph(gemm, args.reps)[0] * 1e3
                ft = {}
                if args.forms:
                    oc = torch.empty(M, inter, dtype=torch.bfloat16, device=dev)
                    for v in FORMS:
                        def forced():
                            f(x.data_ptr(), b4.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), src.data_ptr() if src is not None else None, T,
                              0 if act == "silu" else 1, ACT_ALPHA, LIMIT, bias.data_ptr() if bias is not None else None, oc.data_ptr(), M, N, K, E,
                              torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(fused, args.reps)[0] * 1e3
                tb2 = bench_graph(chain, args.reps)[0] * 1e3
                spread = max(abs(t2 / t - 1), abs(tb2 / tb - 1))
                form, fg = (str(plans[n](M, N, K, E, None)) for n in ("bf16_nvf4_act", "bf16_nvf4"))
                ba = f"{tb / t:.2f}"
                ba = f"**{ba}**" if tb / t < 1 - spread else ba
                line = (f"{model:14s} {act:8s} {phase:8s} {kind:8s} {E:4d} {inter:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {fg:>4s} {tb:9.2f} {tc:9.2f} "
                        f"{t2:9.2f} {tb2:10.2f} {spread:6.3f} {ba:>8s} {tc / t:6.2f}")
                rec = dict(model=model, gather=int(args.gather), act=act, phase=phase, routing=kind, E=E, I=inter, K=K, M=M, form=form, act_us=round(t, 3), act_q20_us=round(lo, 3),
                           act_q80_us=round(hi, 3), act_again_us=round(t2, 3), gemm_form=fg, chain_us=round(tb, 3), chain_again_us=round(tb2, 3), gemm_us=round(tc, 3))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(x_, 3) for v, x_ in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del x, src
        del b4, b_sf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
