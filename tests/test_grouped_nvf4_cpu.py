"""Grouped NVFP4 GEMM (grouped_matmul_nvf4_bf16_tn) on the host: the C entry's declaration and argument checks, the form rule (through
qutlass_amd_debug_grouped_nvf4_plan), the tile decode for the 128-row tiles of its prefill form (tests/test_grouped_cpu.py covers TM = 32 and 64), and the torch
op's fake kernel.  No GPU needed; the GPU half is tests/test_gpu_grouped_nvf4.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_nvf4_bf16_tn"
TILES = {598: (32, 32), 599: (64, 32), 600: (64, 64), 601: (128, 128)}


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    L.qutlass_amd_debug_grouped_nvf4_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_grouped_nvf4_plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    L.qutlass_amd_debug_grouped_decode.restype = ctypes.c_int
    L.qutlass_amd_debug_grouped_decode.argtypes = [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    return L


def test_entry_is_declared_and_exported(lib):
    from qutlass_amd import build

    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    assert re.search(r"\bqutlass_amd_grouped_matmul_nvf4_bf16_tn\s*\(", hdr)
    assert not re.search(r"\bqutlass_amd_debug_grouped_nvf4_plan\b", hdr), "debug entries stay out of the public header"
    assert hasattr(lib, ENTRY)
    from qutlass_amd._lib import SYMBOLS

    assert ENTRY in SYMBOLS
    assert os.path.exists(build.BENCH_OUT), build.BENCH_OUT
    assert hasattr(ctypes.CDLL(build.BENCH_OUT), ENTRY), "the lab library exports the entry too"


def test_entry_rejects_bad_arguments_without_launching(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    d = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    g = getattr(lib, ENTRY)
    err = lambda: lib.qutlass_amd_last_error().decode()

    def call(A=d, B=d, A_sf=d, B_sf=d, alpha=d, n_alpha=1, offs=d, D=d, M=64, N=256, K=512, E=8):
        return g(A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E, None)

    for k in ("A", "B", "A_sf", "B_sf", "alpha", "offs", "D"):
        assert call(**{k: None}) == QAMD_ERR_INVALID, k
        assert "null pointer" in err()
    for E in (0, -1, 1025):
        assert call(E=E) == QAMD_ERR_INVALID and "E must be in [1, 1024]" in err(), E
    for n_alpha in (0, 3, 9):
        assert call(n_alpha=n_alpha) == QAMD_ERR_INVALID and "alpha must have 1 or E" in err(), n_alpha
    assert call(K=96) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(K=640 + 64) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(K=0) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(N=260) == QAMD_ERR_INVALID and "multiple of 8" in err()
    assert call(N=0) == QAMD_ERR_INVALID
    assert call(M=-1) == QAMD_ERR_INVALID
    # one expert of N * K/2 = 2^31 bytes, a token matrix of 2^31 bytes
    assert call(N=16384, K=262144) == QAMD_ERR_INVALID and "one expert's weight" in err() and "below 2 GiB" in err()
    assert call(M=16384, N=256, K=262144) == QAMD_ERR_INVALID and "token matrix" in err() and "below 2 GiB" in err()
    assert call(M=1 << 24, K=256) == QAMD_ERR_INVALID and "token matrix" in err()
    assert call(M=1 << 20, N=1 << 20, K=128) == QAMD_ERR_INVALID and "2^40" in err()
    assert call(M=1 << 23, N=8192, K=128, E=1024) == QAMD_ERR_INVALID and "2^24 workgroups" in err()
    # M == 0: accepted, nothing launched (this machine may have no GPU at all) -- shared and per-expert alpha
    assert call(M=0) == 0
    assert call(M=0, n_alpha=8) == 0
    # just below the 2 GiB limits (M == 0: the checks run, nothing is launched)
    assert call(M=0, N=16376, K=262144) == 0
    assert call(M=0, N=16384, K=262144 - 128) == 0


def _want(M, N, K, E):
    """the mean rows per group M / E pick the tile (<= 48: 64x64, beyond: 128x128); at most 16 rows per group on K >= 8192: the wave-owned kernel"""
    if M <= 16 * E and K >= 8192:
        return 598
    return 600 if M <= 48 * E else 601


def test_plan_follows_the_documented_rule(lib):
    p = lib.qutlass_amd_debug_grouped_nvf4_plan
    grid = ctypes.c_int64()
    shapes = [   # (E, N, K): Qwen3-30B-A3B and Mixtral-8x7B gate/up and down, plus edges
        (128, 1536, 2048), (128, 2048, 768), (8, 28672, 4096), (8, 4096, 14336), (1, 2048, 8192), (256, 512, 8064), (64, 1024, 16384), (1024, 264, 128),
    ]
    for E, N, K in shapes:
        for M in (1, 4 * E, 16 * E, 16 * E + 1, 32 * E, 48 * E, 48 * E + 1, 64 * E, 128 * E, 256 * E, 1024 * E):   # decode and prefill
            v = p(M, N, K, E, ctypes.byref(grid))
            assert v == _want(M, N, K, E), (M, N, K, E, v)
            TM, TN = TILES[v]
            assert grid.value == (-(-M // TM) + E) * (-(-N // TN)), (M, N, K, E)
    assert p(512, 1536, 2048, 128, None) == 600                               # Qwen3 gate/up decode: batch 64 x top-8, 4 rows per expert
    assert p(512, 2048, 768, 128, None) == 600                                # Qwen3 down decode
    assert p(128, 28672, 4096, 8, None) == 600                                # Mixtral gate/up decode: batch 64 x top-2, 16 rows per expert
    assert p(128, 4096, 14336, 8, None) == 598                                # Mixtral down decode: a long K at few rows -> the wave-owned kernel
    assert p(129, 4096, 14336, 8, None) == 600 and p(128, 4096, 8192, 8, None) == 598 and p(128, 4096, 8064, 8, None) == 600
    assert p(8192, 28672, 4096, 8, None) == 601                               # Mixtral gate/up prefill: 1024 rows per expert -> 128x128 tiles
    assert p(32768, 1536, 2048, 128, None) == 601                             # Qwen3 gate/up prefill: 256 rows per expert
    grid.value = -1
    assert p(0, 2048, 768, 8, ctypes.byref(grid)) == _want(0, 2048, 768, 8) and grid.value == 0
    assert p(64, 2048, 4000, 8, None) == -1       # K % 128
    assert p(64, 2044, 4096, 8, None) == -1       # N % 8
    assert p(64, 2048, 4096, 0, None) == -1       # E
    assert p(64, 2048, 4096, 1025, None) == -1
    assert p(64, 16384, 262144, 8, None) == -1    # one expert of 2 GiB
    assert p(-1, 2048, 4096, 8, None) == -1


# ---- the tile decode for TM = 128 (the 128x128 form) -------------------------------------------------------------------------------------------
def _decode(lib, offs, M, TM, tiles_n):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    E = len(offs)
    nwg = (-(-M // TM) + E) * tiles_n         # the host's grid bound
    out = (ctypes.c_int * (4 * nwg))()
    n = lib.qutlass_amd_debug_grouped_decode(offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), E, M, TM, tiles_n, nwg, out)
    return n, np.frombuffer(out, dtype=np.int32).reshape(nwg, 4).copy()


def _coverage(t, n, M, TM, tiles_n, E):
    """rows covered per column tile; the real workgroups are the first n, every (tile, column tile) once"""
    assert (t[:n, 0] >= 0).all() and (t[n:, 0] == -1).all(), "the workgroups without work are the last ones"
    real = t[:n]
    assert len({(g, r0, nt) for g, r0, _, nt in real}) == n
    cover = np.zeros((tiles_n, M), dtype=np.int64)
    for g, r0, rows, nt in real:
        assert 0 <= g < E and 1 <= rows <= TM and 0 <= r0 and r0 + rows <= M and 0 <= nt < tiles_n, (g, r0, rows, nt)
        cover[nt, r0:r0 + rows] += 1
    return real, cover


def _route(rng, M, E, kind):
    if kind == "uniform":
        counts = np.bincount(rng.integers(0, E, M), minlength=E)
    elif kind == "skewed":           # half of the rows in one expert
        counts = np.bincount(rng.integers(0, E, M - M // 2), minlength=E)
        counts[rng.integers(0, E)] += M // 2
    elif kind == "empty":            # most experts get nothing
        live = rng.choice(E, size=max(1, E // 8), replace=False)
        counts = np.zeros(E, dtype=np.int64)
        counts[live] = np.bincount(rng.integers(0, len(live), M), minlength=len(live))
    return np.cumsum(counts)


def _check_wellformed(lib, offs, M, tiles_n=3, TM=128):
    offs = np.asarray(offs, dtype=np.int64)
    E = len(offs)
    n, t = _decode(lib, offs, M, TM, tiles_n)
    starts = np.concatenate([[0], offs[:-1]])
    assert n == tiles_n * sum(-(-(e - s) // TM) for s, e in zip(starts, offs))   # ceil(rows_g / TM) tiles per group and column tile
    real, cover = _coverage(t, n, M, TM, tiles_n, E)
    for g, r0, rows, nt in real:
        assert starts[g] <= r0 and r0 + rows <= offs[g], (g, r0, rows)              # inside its group
    end = int(offs[-1])
    assert (cover[:, :end] == 1).all(), "every row of [0, offs[-1]) exactly once per column tile"
    assert (cover[:, end:] == 0).all(), "rows past offs[-1] are not covered"


def test_decode_for_128_row_tiles_covers_every_row_once(lib):
    rng = np.random.default_rng(11)
    for E in (1, 2, 8, 63, 64, 65, 128, 1000, 1024):
        for M in (1, 127, 128, 129, 1000, 8192):
            for kind in ("uniform", "skewed", "empty"):
                _check_wellformed(lib, _route(rng, M, E, kind), M)
    _check_wellformed(lib, [4096], 4096)                                    # E = 1
    _check_wellformed(lib, _route(rng, 3000, 16, "skewed"), 3000, tiles_n=1)
    _check_wellformed(lib, _route(rng, 3000, 16, "uniform"), 3000, tiles_n=24)
    _check_wellformed(lib, [0] * 7 + [300], 300)                            # everything in the last expert
    _check_wellformed(lib, [300] * 8, 300)                                  # everything in the first
    _check_wellformed(lib, [0] * 16, 256)                                   # all empty
    _check_wellformed(lib, np.minimum(_route(rng, 4000, 128, "uniform"), 2700), 4000)   # offs[-1] < M: rows 2700 ... 3999 untouched


def test_decode_for_128_row_tiles_of_malformed_offsets_stays_inside_m(lib):
    rng = np.random.default_rng(5)
    M = 1031
    cases = [[1200, 10, 20, 1400], [-5, 140, 130, 1 << 30], [M + 1] * 4, [-(1 << 31)] * 3 + [2 ** 31 - 1], [900, 500, 100], [10, -10, 20]]
    for _ in range(100):
        cases.append(rng.integers(-200, M + 400, int(rng.integers(1, 300))))
    for offs in cases:
        E = len(offs)
        n, t = _decode(lib, offs, M, 128, 2)      # (every workgroup index of the grid bound: the decode never goes past it)
        real, cover = _coverage(t, n, M, 128, 2, E)
        assert (cover <= 1).all(), "no row written twice"
        # the clamped running maximum: group g covers [max(clamp(offs[:g])), max(clamp(offs[:g+1])))
        ends = np.maximum.accumulate(np.clip(np.asarray(offs, dtype=np.int64), 0, M))
        starts = np.concatenate([[0], ends[:-1]])
        for g, r0, rows, nt in real:
            assert starts[g] <= r0 and r0 + rows <= ends[g], (g, r0, rows)
        assert (cover[:, :ends[-1]] == 1).all() and (cover[:, ends[-1]:] == 0).all()


def test_fake_kernel_and_aot_graph():
    from torch._dynamo.backends.common import aot_autograd
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass  # the drop-in alias reaches the extension too
    import qutlass_amd as q

    assert qutlass.grouped_matmul_nvf4_bf16_tn is q.grouped_matmul_nvf4_bf16_tn
    assert q.grouped_matmul_nvf4_bf16_tn.__doc__.startswith("EXTENSION")
    assert "grouped_matmul_nvf4_bf16_tn" in q.__doc__
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_nvf4").fake_impl.kernel is not None
    M, N, K, E = 96, 256, 512, 4
    e4 = torch.float8_e4m3fn
    with FakeTensorMode():
        a = torch.empty(M, K // 2, dtype=torch.uint8, device=DEV)
        b = torch.empty(E, N, K // 2, dtype=torch.uint8, device=DEV)
        a_sf = torch.empty(M * K // 16, dtype=e4, device=DEV)
        b_sf = torch.empty(E * N * K // 16, dtype=e4, device=DEV)
        alpha = torch.empty(E, device=DEV)
        offs = torch.empty(E, dtype=torch.int32, device=DEV)
        out = q.grouped_matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs) * 2

    args = (torch.zeros(M, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 2, dtype=torch.uint8),
            torch.zeros(M * K // 16, dtype=torch.uint8).view(e4), torch.zeros(E * N * K // 16, dtype=torch.uint8).view(e4),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32))

    gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_nvf4.default" in targets, targets

    graphs = []

    def capture(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    torch._dynamo.reset()
    try:   # CPU tensors: tracing never looks at the device, and the run after it has no kernel to call (CUDA key only) -- the graph exists by then
        torch.compile(layer, backend=aot_autograd(fw_compiler=capture), fullgraph=True)(*args)
    except (NotImplementedError, RuntimeError) as e:
        assert graphs and ("CPU" in str(e) or "backend" in str(e)), e
    assert graphs
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_nvf4.default" in targets, targets
