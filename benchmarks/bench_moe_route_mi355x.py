#!/usr/bin/env python3
"""MoE routing -- router logits to expert ids, weights and the sorted-row metadata -- each op against the torch composition it replaces.

  topk    ours_us   one launch: moe_topk_softmax(logits, topk)
          torch_us  softmax(logits.float()) -> topk -> divide by the selected sum
  sort    ours_us   moe_sort_fused(ids, E): one launch up to the one-launch bound, three beyond
          torch_us  moe_sort(ids, E) (stable argsort, searchsorted, scatter, where, div, casts)
  route   ours_us   moe_route(logits, topk)
          torch_us  the torch top-k composition followed by moe_sort
  bound   one_us / three_us: the one-workgroup and the three-launch form of the sort of the SAME (lab) build on the same ids, forced through the lab library's
          "moe_sort_one_launch_max" option -- the one-launch bound of the product is where three_us first drops below one_us

Every point is taken twice: `graph` -- medians of HIP-graph replays (bench_configs.time_us: device time, no host work between the launches) -- and `eager` -- a host
clock around back-to-back calls ending in a synchronise (what a caller without graphs pays, Python and launch overhead included).  `spread` / `torch_spread` (and
`one_spread` / `three_spread` of the bound step) are (max - min) / median of each side over --repeat whole measurements; ours and torch alternate inside every repeat.
A gain or a crossover counts only where it exceeds both spreads.

Shapes: Mixtral-8x7B (E = 8, top-2) and Qwen3-30B-A3B (E = 128, top-8) at T in {1, 16, 64, 512, 4096, 16384}, bf16 logits.

Every (model, phase) is one GPU step: a child process of its own under its own time limit (--step-timeout), and the first step that fails or runs out of time ends the
run -- nothing more is started on a device that has just misbehaved.

    python benchmarks/bench_moe_route_mi355x.py [--repeat 3] [--quick] [--step-timeout 300]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (model, E, top-k)
MODELS = [("Mixtral-8x7B", 8, 2), ("Qwen3-30B-A3B", 128, 8)]
TOKENS = {"decode": [1, 16, 64], "prefill": [512, 4096, 16384]}
STEPS = [(m, p) for m in range(len(MODELS)) for p in TOKENS] + [(m, "bound") for m in range(len(MODELS))]
BOUND_SLOTS = [1024, 2048, 4096, 6144, 8192, 12288, 16384, 32768, 65536, 131072]


def time_eager_us(fn, iters):
    import torch

    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def torch_topk(logits, topk):
    import torch

    p = torch.softmax(logits.float(), dim=-1)
    w, ids = torch.topk(p, topk, dim=-1)
    return w / w.sum(dim=-1, keepdim=True), ids


def run_step(model_i, phase, args):
    import numpy as np
    import torch

    from bench_configs import time_us
    import qutlass_amd as q

    dev = torch.device("cuda:0")
    model, E, topk = MODELS[model_i]
    print(f"# {q._lib.load().qutlass_amd_version().decode()}  {torch.cuda.get_device_name(0)}  iters={args.iters} repeat={args.repeat}", flush=True)

    def measure(fa, fb):
        res = {}
        for mode in ("graph", "eager"):
            t = (lambda f: time_us(f, args.iters)) if mode == "graph" else (lambda f: time_eager_us(f, args.iters))
            ta, tb = [], []
            for _ in range(max(1, args.repeat)):
                ta.append(t(fa))
                tb.append(t(fb))
            a_, b_ = float(np.median(ta)), float(np.median(tb))
            res[mode] = (a_, b_, (max(ta) - min(ta)) / a_, (max(tb) - min(tb)) / b_)
        return res

    def report(op, T, res, extra=None):
        for mode, (a_, b_, spread, tspread) in res.items():
            print(f"{op:5s} {model:14s} {phase:8s} T={T:6d} E={E:4d} topk={topk} {mode:>5s} ours_us {a_:9.2f} torch_us {b_:9.2f} torch/ours {b_ / a_:6.2f} spread {spread:5.3f} torch_spread {tspread:5.3f}", flush=True)
            print("JSON " + json.dumps(dict(op=op, model=model, phase=phase, T=T, E=E, topk=topk, mode=mode, ours_us=round(a_, 3), torch_us=round(b_, 3),
                                            spread=round(spread, 4), torch_spread=round(tspread, 4), **(extra or {}))), flush=True)

    if phase == "bound":
        return run_bound(model, E, topk, args, time_us)
    for T in TOKENS[phase]:
        if args.quick and T not in (16, 4096):
            continue
        gen = torch.Generator(device="cpu").manual_seed(T)
        logits = (torch.randn(T, E, generator=gen) * 3.0).to(torch.bfloat16).to(dev)
        _, ids = q.moe_topk_softmax(logits, topk)
        ids64 = ids.long()
        report("topk", T, measure(lambda: q.moe_topk_softmax(logits, topk), lambda: torch_topk(logits, topk)))
        report("sort", T, measure(lambda: q.moe_sort_fused(ids, E), lambda: q.moe_sort(ids64, E)),
               dict(launches=1 if q._lib.load().qutlass_amd_moe_sort_workspace_bytes(T * topk, E) == 0 else 3))
        report("route", T, measure(lambda: q.moe_route(logits, topk), lambda: q.moe_sort(torch_topk(logits, topk)[1], E)))


def run_bound(model, E, topk, args, time_us):
    """one workgroup against three launches, same lab build, same ids: C-ABI calls on the current stream (what csrc/torch_ext.cpp does for the product)"""
    import numpy as np
    import torch

    lab = ctypes.CDLL(os.path.join(ROOT, "qutlass_amd", "libqutlass_amd_bench.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lab.qutlass_amd_moe_sort.restype, lab.qutlass_amd_moe_sort.argtypes = i32, [vp, i32, i64, i64, i64, vp, i64, vp, vp, vp, vp, i64, vp]
    lab.qutlass_amd_moe_sort_workspace_bytes.restype, lab.qutlass_amd_moe_sort_workspace_bytes.argtypes = i64, [i64, i64]
    lab.qutlass_amd_set_option.restype, lab.qutlass_amd_set_option.argtypes = i32, [ctypes.c_char_p, i32]
    dev = torch.device("cuda:0")
    for n in BOUND_SLOTS:
        T = n // topk
        ids = torch.from_numpy(np.random.default_rng(n).integers(0, E, (T, topk)).astype(np.int32)).to(dev)
        out = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
        res, ref = {}, None
        for form, opt in (("one", 1 << 30), ("three", 1)):
            lab.qutlass_amd_set_option(b"moe_sort_one_launch_max", opt)
            wsb = lab.qutlass_amd_moe_sort_workspace_bytes(n, E)
            assert (wsb == 0) == (form == "one")
            ws = torch.empty(max(wsb, 4) // 4, dtype=torch.int32, device=dev)

            def call():
                rc = lab.qutlass_amd_moe_sort(ids.data_ptr(), 4, T, topk, E, None, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                              ws.data_ptr() if wsb else None, wsb, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc

            call()
            torch.cuda.synchronize()
            got = [o.clone() for o in out]
            ref = ref or got
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), "the two forms differ"
            res[form] = [time_us(call, args.iters) for _ in range(max(1, args.repeat))]
        lab.qutlass_amd_set_option(b"moe_sort_one_launch_max", 0)
        one, three = float(np.median(res["one"])), float(np.median(res["three"]))
        s1, s3 = (max(res["one"]) - min(res["one"])) / one, (max(res["three"]) - min(res["three"])) / three
        print(f"bound {model:14s} n={n:7d} E={E:4d} graph one_us {one:8.2f} three_us {three:8.2f} one/three {one / three:5.2f} one_spread {s1:5.3f} three_spread {s3:5.3f}", flush=True)
        print("JSON " + json.dumps(dict(op="bound", model=model, n=n, E=E, one_us=round(one, 3), three_us=round(three, 3), one_spread=round(s1, 4), three_spread=round(s3, 4))),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per row (ours and the torch form alternate); medians are reported")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="T = 16 and 4096 only, no bound sweep")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one (model, phase) step may take")
    ap.add_argument("--step", type=int, default=-1, help=argparse.SUPPRESS)   # (internal: run this one step in this process)
    args = ap.parse_args()
    if args.step >= 0:
        run_step(*STEPS[args.step], args)
        return 0
    for i, (m, phase) in enumerate(STEPS):
        if args.quick and phase == "bound":
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(i), "--repeat", str(args.repeat), "--iters", str(args.iters)] + (["--quick"] if args.quick else [])
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"step {MODELS[m][0]} {phase}: no result within {args.step_timeout} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"step {MODELS[m][0]} {phase}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
