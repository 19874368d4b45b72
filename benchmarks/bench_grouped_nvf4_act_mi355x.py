#!/usr/bin/env python3
"""The gate/up NVFP4 (W4A4) grouped GEMM with fused activation, rotation and NVFP4 output (qutlass_amd.grouped_matmul_nvf4_silu_nvf4_tn / ..._swiglu_oai_nvf4_tn) against
the launches it replaces, on the same tokens, expert weights and routing (graph-timed like benchmarks/bench_grouped_mxf4_act_mi355x.py: median of HIP-graph replays):

    act_us       (a) the fused op, the form its rule picks; q20 / q80 beside it
    act_2_us     the same measurement taken a second time after the other columns: the run-to-run spread of this table (the "two takes" of a cell)
    chain_us     (b) grouped_matmul_nvf4_bf16_tn, then fusedSiluMulQuantizeNvGrouped -- or, for the clamped SwiGLU with bias, swiglu_oai_and_mul and
                 fusedGatherQuantizeNvGrouped (three launches) -- on its output with the same h (a signed Hadamard matrix of 32), global scales and method
    gemm_us      (c) grouped_matmul_nvf4_bf16_tn alone (fg: its form; 600 / 601 are the tile bodies forms 624 / 625 mirror): chain_us - gemm_us is what the saved
                 launches cost, gemm_us - act_us what the fused epilogue gains or loses against the GEMM's own
    b/a, c/a     chain_us / act_us and gemm_us / act_us: above 1 the fused op is faster; a loser is printed in **bold**
    --forms      also both forms forced through the lab library (624 = 64 rows x 32 activation columns, 625 = 128 x 64): the calibration of the form rule
                 (qutlass_amd/csrc/capi.hip grouped_nvf4_act_plan)

Cells: the gate/up projections of gpt-oss-20b / 120b (clamped SwiGLU with bias; I = H = 2944, 2880 padded to K % 128 == 0), Qwen3-30B-A3B and Mixtral-8x7B (silu), at
16 and 64 tokens (decode) and 4096 (prefill), uniform and skewed routing.  Operands are random codes with scale bytes near 1.0 (timing only).

    --sweep      instead of the models: 128 experts, I = 1024, silu, a mean of 16 ... 128 rows per expert at K = 768 ... 3328 -- around the rule's threshold of 48 rows

    python benchmarks/bench_grouped_nvf4_act_mi355x.py [--reps 50] [--forms] [--quick] [--only SUBSTRING] [--sweep] [--method quest|abs_max]
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
FORMS = (624, 625)
SWEEP_ROWS, SWEEP_K = (16, 32, 48, 64, 128), (768, 1024, 2048, 3328)
ACT_ALPHA, LIMIT = 1.702, 7.0


def ratio(x, t):
    """x / t, bold where the fused op (t) loses"""
    s = f"{x / t:.2f}"
    return f"{'**' + s + '**' if x < t else s:>8s}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forms", action="store_true", help="also time both forms forced through the lab library")
    ap.add_argument("--quick", action="store_true", help="decode only, uniform routing")
    ap.add_argument("--only", default="", help="only the models whose name contains this")
    ap.add_argument("--sweep", action="store_true", help="rows per expert x K around the form rule's threshold instead of the models")
    ap.add_argument("--method", default="abs_max", choices=("quest", "abs_max"))
    args = ap.parse_args()
    import _rotations
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    lab = None
    if args.forms:
        import _benchlib as lab

        f = lab.load().qutlass_amd_grouped_matmul_nvf4_act_nvf4_tn
        f.restype = ctypes.c_int
        f.argtypes = q._lib.SYMBOLS["qutlass_amd_grouped_matmul_nvf4_act_nvf4_tn"][1]
    plans = {}
    for name in ("grouped_nvf4_act", "grouped_nvf4"):
        fp = getattr(q._lib.load(), f"qutlass_amd_debug_{name}_plan")
        fp.restype = ctypes.c_int
        fp.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_void_p]
        plans[name] = fp
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  reps={args.reps}  method={args.method}")
    hdr = (f"{'model':14s} {'act':8s} {'phase':8s} {'routing':8s} {'E':>4s} {'I':>6s} {'K':>6s} {'M':>6s} {'form':>5s} {'act_us':>9s} {'q20':>8s} {'q80':>8s} {'act_2_us':>9s} "
           f"{'fg':>4s} {'chain_us':>9s} {'b/a':>8s} {'gemm_us':>9s} {'c/a':>8s}")
    if args.forms:
        hdr += "  " + " ".join(f"{v:>8d}" for v in FORMS)
    print(hdr)
    gen = torch.Generator(device=dev).manual_seed(0)
    h = _rotations.signed_permuted_hadamard(32).to(dev)
    method = args.method
    layers = [("sweep", "silu", 128, 1024, K, 1) for K in SWEEP_K] if args.sweep else LAYERS
    tokens = {f"r{r}": 128 * r for r in SWEEP_ROWS} if args.sweep else TOKENS
    e4m3 = torch.float8_e4m3fn
    for model, act, E, inter, K, topk in layers:
        if args.only and args.only not in model:
            continue
        kb, N = K // 16, 2 * inter
        b4 = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        b_sf = torch.randint(0x30, 0x40, (E * N * kb,), dtype=torch.uint8, device=dev, generator=gen).view(e4m3)
        bias = torch.randn(E, N, device=dev, generator=gen).to(torch.bfloat16) if act == "oai_bias" else None
        gs = torch.rand(E, device=dev, generator=gen) + 0.5
        for phase, T in tokens.items():
            if args.quick and not phase.startswith("decode"):
                continue
            M = T * topk
            a4 = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=gen)
            a_sf = torch.randint(0x30, 0x40, (M * kb,), dtype=torch.uint8, device=dev, generator=gen).view(e4m3)
            alpha = torch.full((1,), 2.0 ** -8, device=dev)
            rows = torch.arange(M, dtype=torch.int32, device=dev)
            for kind in ("uniform", "skewed"):
                if (args.quick or args.sweep) and kind != "uniform":
                    continue
                c = routing(M, E, kind)
                offs = torch.tensor(np.cumsum(c), dtype=torch.int32, device=dev)

                def gemm():
                    return q.grouped_matmul_nvf4_bf16_tn(a4, b4, a_sf, b_sf, alpha, offs)

                if act == "silu":
                    def fused():
                        q.grouped_matmul_nvf4_silu_nvf4_tn(a4, b4, a_sf, b_sf, alpha, offs, h, gs, method=method)

                    def chain():
                        q.fusedSiluMulQuantizeNvGrouped(gemm(), h, gs, offs, method=method)
                else:
                    def fused():
                        q.grouped_matmul_nvf4_swiglu_oai_nvf4_tn(a4, b4, a_sf, b_sf, alpha, offs, h, gs, method=method, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias)

                    def chain():
                        q.fusedGatherQuantizeNvGrouped(q.swiglu_oai_and_mul(gemm(), alpha=ACT_ALPHA, limit=LIMIT, bias=bias, offs=offs), h, gs, rows, offs, method=method)

                t, lo, hi = (x * 1e3 for x in bench_graph(fused, args.reps)[:3])
                tb = bench_graph(chain, args.reps)[0] * 1e3
                tc = bench_graph(gemm, args.reps)[0] * 1e3
                ft = {}
                if args.forms:
                    oc = torch.empty(M, inter // 2, dtype=torch.uint8, device=dev)
                    osf = torch.empty(M * inter // 16, dtype=torch.uint8, device=dev)
                    for v in FORMS:
                        def forced():
                            f(a4.data_ptr(), b4.data_ptr(), a_sf.data_ptr(), b_sf.data_ptr(), alpha.data_ptr(), 1, offs.data_ptr(), 0 if act == "silu" else 1, ACT_ALPHA, LIMIT,
                              bias.data_ptr() if bias is not None else None, h.data_ptr(), 32, gs.data_ptr(), 0 if method == "quest" else 1, oc.data_ptr(), osf.data_ptr(),
                              M, N, K, E, torch.cuda.current_stream().cuda_stream)
                        with lab.forced(gemm_variant=v):
                            ft[v] = bench_graph(forced, args.reps)[0] * 1e3
                t2 = bench_graph(fused, args.reps)[0] * 1e3
                form, fg = (str(plans[n](M, N, K, E, None)) for n in ("grouped_nvf4_act", "grouped_nvf4"))
                line = (f"{model:14s} {act:8s} {phase:8s} {kind:8s} {E:4d} {inter:6d} {K:6d} {M:6d} {form:>5s} {t:9.2f} {lo:8.2f} {hi:8.2f} {t2:9.2f} {fg:>4s} {tb:9.2f} "
                        f"{ratio(tb, t)} {tc:9.2f} {ratio(tc, t)}")
                rec = dict(model=model, act=act, phase=phase, routing=kind, E=E, I=inter, K=K, M=M, form=form, act_us=round(t, 3), act_q20_us=round(lo, 3), act_q80_us=round(hi, 3),
                           act_again_us=round(t2, 3), gemm_form=fg, chain_us=round(tb, 3), gemm_us=round(tc, 3))
                if args.forms:
                    line += "  " + " ".join(f"{ft[v]:8.2f}" for v in FORMS)
                    rec["forms_us"] = {str(v): round(x, 3) for v, x in ft.items()}
                print(line, flush=True)
                print("JSON " + json.dumps(rec), flush=True)
            del a4, a_sf
        del b4, b_sf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
