"""Forms, shapes and operand builders shared by tests/test_mx_scale_range_cpu.py (no GPU), tests/test_gpu_mx_scale_range.py and tests/test_gpu_gemm_footprint.py.

A CASE is one kernel form of one MX GEMM op at one shape: (op, a5, variant, lab options, m, n, k).
  op       "mxf4" matmul_mxf4_bf16_tn (_ws entry) | "mxf8" matmul_mxf8_bf16_tn (_fmt entry) | "ada" matmul_ada_mxf4_bf16_tn (row-major scales) |
           "nn" matmul_mxf8_bf16_nn (_fmt entry; A stored (K, M)) | "g4" / "g8" grouped_matmul_mxf{4,8}_bf16_tn (m = token rows over GROUPED_E experts, offs[-1] == m) |
           "g48" grouped_matmul_mxf8_mxf4_bf16_tn (W4A8: e4m3 tokens against e2m1 weights; its reference is tests/_w4a8_model.py, the oracle has no mixed kind)
  a5       MXFP8 only: A in e5m2
  variant  the lab library's "gemm_variant" (the MxVariant numbers of csrc/gemm_mx_forms.hip.h MX_FORMS, which tests read through qutlass_amd_debug_mx_forms; 62 / 63: the two operand paths of the NN op; 590 ... 597, 602 ... 604: the grouped forms)
  options  further lab options: deepp_grid (persistent workgroups, so that each walks several tiles), splitk_force (K ranges of a forced ring tile: the _ws entry with scratch)

Shapes are the smallest at which a form can still go wrong: two tiles plus a ragged remainder in M (not a multiple of 16) and in N (a multiple of 8, not of the tile), a K
of 9.5 stages of 128 bytes per row (9.25 for MXFP8: K % 128 == 32, the last scale dword partly past K) so that 3- and 4-deep rings wrap twice, and for the forms whose
kernel depends on K (one-shot / wave-owned rings, the two ring depths of 561 / 562, the odd-stage-count form of the persistent kernel) one K on each side.

The lab-only stream-K walk (variant 89) is left out: no product plan returns it (test_mx_scale_range_cpu.py pins that), and it cannot be entered below 257 tiles of 256x256.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import oracle

SENTINEL = 0x7FC1            # bf16 NaN payload no kernel produces: the guard rows around D and the unwritten state of D
GUARD_ROWS = 256             # one tile of the largest form
WS_TAIL = 1 << 20
GROUPED_E = 4
EXACT_VALS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0], np.float32)   # tests/test_gpu_round6.py: the exact regime of fp8 codes


class Case(NamedTuple):
    op: str
    a5: bool
    variant: int
    opts: tuple
    m: int
    n: int
    k: int

    @property
    def id(self):
        o = "".join(f"-{k}{v}" for k, v in self.opts)
        return f"{self.op}{'-a5' if self.a5 else ''}-v{self.variant}{o}-{self.m}x{self.n}x{self.k}"

    @property
    def fp8(self):
        return self.op in ("mxf8", "nn", "g8", "g48")      # (the A operand: "g48" has e2m1 weights)

    @property
    def grouped(self):
        return self.op in ("g4", "g8", "g48")


T256, T128, T64, T32, T64N = (531, 552), (275, 296), (147, 168), (83, 200), (147, 200)
G = ("deepp_grid", 2)


def _sf(n):
    return ("splitk_force", n)


# (variant, options, (m, n), K list for MXFP4, K list for MXFP8) -- the TN forms both element widths have
_TN = [
    (90, (G,), T256, (2432, 2176), (1184,)),      # persistent 256x256, several tiles per workgroup; MXFP4: even and odd stage counts (gemm_mx_deepp ODD)
    (90, (), T256, (2432, 2176), (1184,)),        # ... one tile per workgroup (ONETILE)
    (98, (G,), T256, (2432, 2176), (1184,)),      # heterogeneous launch: 8 tiles on 2 persistent workgroups + 4 quarter tiles
    (25, (), T256, (2432,), (1184,)), (58, (), T256, (2432,), (1184,)),
    (24, (), T128, (2432,), (1184,)), (27, (), T128, (2432,), (1184,)), (28, (), T128, (2432,), (1184,)), (29, (), T64, (2432,), (1184,)),
    (70, (), T64, (2432,), (1184,)), (71, (), T128, (2432,), (1184,)), (72, (), T128, (2432,), (1184,)), (73, (), T128, (2432,), (1184,)),
    (70, (_sf(2),), T64, (2432,), (1184,)), (70, (_sf(3),), T64, (2432,), (1184,)), (72, (_sf(2),), T128, (2432,), (1184,)), (73, (_sf(3),), T128, (2432,), (1184,)),
    (73, (_sf(8),), T128, (2432,), (1184,)),      # split-K over caller scratch + splitk_reduce_kernel (5 non-empty K ranges of the 10 stages)
    (568, (), T32, (1408, 4352), (672, 2208)), (569, (), T32, (1408, 4352), (672, 2208)),      # one shot up to 16 stages, wave-owned rings beyond
    (570, (), T64N, (1408, 3328), (672, 1696)),                                                # ... up to 12 stages
    (571, (), T32, (1408, 8448), (672, 4256)),                                                 # decode form, 16 columns: one shot up to 32 stages
    (572, (), T32, (1408, 4352), (672, 2208)), (573, (), T32, (1408, 4352), (672, 2208)), (574, (), T32, (1408, 4352), (672, 2208)),
    (575, (), T32, (1408, 3328), (672, 1696)),
]
_MXF4_ONLY = [(60, (), T32, (2432,)), (561, (), T32, (2432, 6528)), (562, (), T32, (2432, 6528))]   # 561 / 562: 4-deep ring up to 24 stages, 6-deep beyond
_ADA = [60, 70] + list(range(568, 576))
_GROUPED4 = [(590, (1408, 4352)), (591, (1408, 4352)), (592, (1408, 3328)), (593, (2432,))]
_GROUPED8 = [(594, (640, 2176)), (595, (640, 2176)), (596, (640, 1664)), (597, (1152,))]            # (the grouped ops take K % 128 == 0 only)
_GROUPED48 = [(602, (3072, 3200)), (603, (3072, 3200)), (604, (1536, 1664))]   # a stage is 128 elements: one shot up to 6 slots per wave (604: up to K = 1536), rings beyond (tests/test_gpu_grouped_w4a8.py)


def _build_cases():
    out = []
    for v, o, (m, n), k4, k8 in _TN:
        out += [Case("mxf4", False, v, o, m, n, k) for k in k4]
        out += [Case("mxf8", a5, v, o, m, n, k) for a5 in (False, True) for k in k8]
    for v, o, (m, n), k4 in _MXF4_ONLY:
        out += [Case("mxf4", False, v, o, m, n, k) for k in k4]
    by_variant = {v: ((m, n), k4) for v, o, (m, n), k4, _ in _TN if not o}
    by_variant[60] = (T32, (2432,))
    for v in _ADA:
        (m, n), k4 = by_variant[v]
        out += [Case("ada", False, v, (), m, n, k) for k in k4]
    for a5 in (False, True):
        out.append(Case("nn", a5, 63, (G,), 528, 552, 1184))    # the persistent kernel reading the (K, M) operand through transposing LDS reads
        out.append(Case("nn", a5, 62, (), 528, 552, 1184))      # byte-transpose pre-pass into the workspace + the TN plan of the shape
        out.append(Case("nn", a5, 62, (), 80, 200, 672))        # ... a small-batch TN plan behind it
    for v, ks in _GROUPED4:
        out += [Case("g4", False, v, (), 300, 200, k) for k in ks]
    for v, ks in _GROUPED8:
        out += [Case("g8", a5, v, (), 300, 200, k) for a5 in (False, True) for k in ks]
    for v, ks in _GROUPED48:
        out += [Case("g48", False, v, (), 300, 200, k) for k in ks]
    return out


CASES = _build_cases()
FP8_CASES = [c for c in CASES if c.fp8]


def covered(op, split=False):
    """variants of an op that CASES runs (split: with more than one K range)"""
    return {c.variant for c in CASES if c.op == op and (not split or any(k == "splitk_force" for k, _ in c.opts))}


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def pad128(r):
    return -(-r // 128) * 128


def isnan_bf16(bits):
    return (np.asarray(bits) & 0x7FFF) > 0x7F80


def _codes(c: Case, rows, rng, e5m2, weights=False):
    if not c.fp8 or (weights and c.op == "g48"):
        return rng.integers(0, 256, size=(rows, c.k // 2), dtype=np.uint8)
    import torch

    v = torch.from_numpy(EXACT_VALS[rng.integers(0, len(EXACT_VALS), size=(rows, c.k))])
    return v.to(torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn).view(torch.uint8).numpy()


def group_counts(c: Case):
    """rows per expert of a grouped case: an empty expert, a one-row expert, boundaries off every tile multiple; sums to m"""
    cnt = [0, 1, 130, c.m - 131]
    assert len(cnt) == GROUPED_E and sum(cnt) == c.m and min(cnt) >= 0
    return cnt


def scale_walk(kb, layout):
    """w(g) of the whole-range layouts, 0 ... 253.  "sweep": 97 g mod 254 walks the whole range in large steps (neighbouring K groups are far apart);
    "extremes": 0, 1, 127, 252, 253 in adjacent groups."""
    g = np.arange(kb)
    if layout == "sweep":
        return (97 * g) % 254
    return np.array([0, 1, 127, 252, 253])[g % 5]


class Data(NamedTuple):
    a: np.ndarray        # (m, k or k/2) codes, row-major (the NN op gets the transpose)
    b: np.ndarray        # (n, ...) codes; grouped: (E n, ...)
    sa: np.ndarray       # (pad128(m), k/32) e8m0 bytes, row-major: rows >= m are what the padding rows of the blocked image hold
    sb: np.ndarray       # (pad128(n), k/32); grouped: (E n, k/32)
    ref: np.ndarray      # (m, n) bf16 bits of the oracle
    alpha: float


def _reference(c: Case, a, b, sa, sb, alpha):
    kind = oracle.KIND_MXFP4 if not c.fp8 else oracle.KIND_MXFP8_TN_A5 if c.a5 else oracle.KIND_MXFP8_TN
    if c.op == "g48":   # fp64 dequantise, matmul, one rounding
        import _w4a8_model as W

        kb = c.k // 32
        p = W.W4A8(a, b.reshape(GROUPED_E, c.n, c.k // 2), sa, sb.reshape(GROUPED_E, c.n, kb))
        return W.to_bf16_bits(W.reference_f64(p, group_counts(c), alpha)).numpy().view(np.uint16)
    if not c.grouped:
        return oracle.gemm_blockscaled(kind, a, b, oracle.to_blocked(sa[:c.m]), oracle.to_blocked(sb[:c.n]), alpha, c.m, c.n, c.k)
    ref = np.empty((c.m, c.n), np.uint16)
    r0 = 0
    for e, cnt in enumerate(group_counts(c)):
        if cnt:
            be, sbe = b[e * c.n:(e + 1) * c.n], sb[e * c.n:(e + 1) * c.n]
            ref[r0:r0 + cnt] = oracle.gemm_blockscaled(kind, a[r0:r0 + cnt], be, oracle.to_blocked(sa[r0:r0 + cnt]), oracle.to_blocked(sbe), alpha, cnt, c.n, c.k)
        r0 += cnt
    return ref


def nan_pattern(c: Case):
    """the predicted isnan(D) of the tracer data: an output is NaN exactly when its A row or its B column touched a poisoned K group"""
    r, col = np.arange(c.m), np.arange(c.n)
    return np.isin(r % 5, (1, 3))[:, None] | (col % 7 == 2)[None, :]


@functools.lru_cache(maxsize=None)
def _dataset(key: Case, part: str) -> Data:
    """key: a case with variant 0 and no options -- forms that share (op, a5, shape) share the operands and the reference"""
    c = key
    grouped = c.grouped
    rng = np.random.default_rng(zlib.crc32(repr((c.op, c.a5, c.m, c.n, c.k, part)).encode()))
    kb = c.k // 32
    rows_a, rows_b = (c.m, GROUPED_E * c.n) if grouped else (pad128(c.m), pad128(c.n))
    nb = rows_b if grouped else c.n
    a, b = _codes(c, c.m, rng, c.a5), _codes(c, nb, rng, False, weights=True)
    ra, rb = np.arange(rows_a)[:, None], np.arange(rows_b)[:, None]
    alpha = 0.5
    if part in ("sweep", "extremes"):
        # sA(r, g) = w(g) + u(r), sB(c, g) = 253 - w(g) + v(c) with u, v in {0, 1}: every block's scale product is 2^-1 ... 2^1 while the bytes of both operands
        # run over 0 ... 254 along K.  (A byte that also swept 0 ... 254 over the ROWS at a fixed K group could not meet one shared B scale with an ordinary product:
        # the row part is the hash u(r), which any wrong scale row still turns into a factor of 2 in that row's outputs.)
        w = scale_walk(kb, part)[None, :]
        sa = (w + (ra * 7 + ra // 32) % 2).astype(np.uint8)
        sb = (253 - w + (rb * 5 + rb // 16) % 2).astype(np.uint8)
    else:
        sa = rng.integers(125, 130, size=(rows_a, kb), dtype=np.uint8)
        sb = rng.integers(125, 130, size=(rows_b, kb), dtype=np.uint8)
    if part == "nan":   # byte 255 = e8m0 NaN as a tracer, continued through the padding rows of the blocked image
        sa[(ra[:, 0] % 5) == 1, min(1, kb - 1)] = 255
        sa[(ra[:, 0] % 5) == 3, kb - 1] = 255
        sb[((rb[:, 0] % c.n if grouped else rb[:, 0]) % 7) == 2, kb // 2] = 255
    if part == "special":
        assert c.fp8 and c.m >= 80 and c.k >= 640
        nanp, nanm = (0x7D, 0xFE) if c.a5 else (0x7F, 0xFF)
        a[2, 5], a[c.m - 1, c.k - 1] = nanp, nanm                     # NaN of both signs in A: first tile, the ragged last row and the last K byte
        if c.op != "g48":                                             # (e2m1 weights have no NaN code)
            b[(2 * c.n if grouped else 0) + 3, 40], b[nb - 1, c.k - 2] = 0x7F, 0xFF   # ... and in B (grouped: the third and the last expert)
        if c.a5:
            a[c.m - 2, 7], a[c.m - 2, 300] = 0x7E, 0x7F               # the other two e5m2 NaN codes
            col = np.arange(nb) % c.n
            one = np.where(col % 2 == 0, 0x38, 0xB8).astype(np.uint8)   # e4m3 +-1.0
            a[17, 33], b[:, 33] = 0x7C, 0x38                          # +inf against +1.0 everywhere ...
            b[col % 11 == 4, 33] = 0x00                     # ... and against a zero code: inf x 0 = NaN in those columns
            a[40, 70], b[:, 70] = 0xFC, one                           # -inf against +-1.0: one infinite product per output, its sign by the column
            a[64, 100], a[64, c.k - 100] = 0x7C, 0xFC                 # +inf and -inf in one row, both against +1.0: inf - inf = NaN in every column
            b[:, 100], b[:, c.k - 100] = 0x38, 0x38
    return Data(a, b, sa, sb, _reference(c, a, b, sa, sb, alpha), alpha)


def dataset(c: Case, part: str) -> Data:
    return _dataset(c._replace(variant=0, opts=(), op={"ada": "mxf4", "nn": "mxf8"}.get(c.op, c.op)), part)


def f32_to_bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def sums_in_fp32(c: Case, d: Data, reverse: bool):
    """sampled outputs with the K groups' block sums added one by one in fp32, forward or reversed: equal bits for both orders = the exact regime
    ("g48": the first and last rows of every expert, each against its own expert's weights)"""
    assert c.op in ("mxf4", "mxf8", "g48")
    bounds = np.r_[0, np.cumsum(group_counts(c))] if c.grouped else np.array([0, c.m])
    segs = [(e, int(r0), int(r1)) for e, (r0, r1) in enumerate(zip(bounds[:-1], bounds[1:])) if r1 > r0]
    rows = np.unique(np.concatenate([np.r_[r0:min(r0 + 8, r1), max(r1 - 8, r0):r1] for _, r0, r1 in segs]))
    cols = np.unique(np.r_[0:16, c.n - 16:c.n])
    kb = c.k // 32
    dec = np.array([oracle.lib().orc_e2m1_decode(i) for i in range(16)], np.float64)
    dec8 = np.array([oracle.lib().orc_e4m3_decode(i) for i in range(256)], np.float64)
    dec5 = np.array([oracle.lib().orc_e5m2_decode(i) for i in range(256)], np.float64)
    unpack = lambda x: np.stack([dec[x & 15], dec[x >> 4]], -1).reshape(x.shape[0], -1)
    av = (dec5 if c.a5 else dec8)[d.a[rows]] if c.fp8 else unpack(d.a[rows])
    acc = np.zeros((len(rows), len(cols)), np.float32)
    for ex, r0, r1 in segs:
        sel, bsel = (rows >= r0) & (rows < r1), ex * c.n + cols
        bv = unpack(d.b[bsel]) if c.op in ("mxf4", "g48") else dec8[d.b[bsel]]
        blk = np.einsum("rgi,cgi->rcg", av[sel].reshape(-1, kb, 32), bv.reshape(len(cols), kb, 32))          # exact: small integers / 4
        e = d.sa[rows[sel]].astype(np.int64)[:, None, :] + d.sb[bsel].astype(np.int64)[None, :, :] - 254
        terms = np.ldexp(blk, e).astype(np.float32)
        assert np.array_equal(terms.astype(np.float64), np.ldexp(blk, e))
        part = np.zeros(terms.shape[:2], np.float32)
        for g in (range(kb - 1, -1, -1) if reverse else range(kb)):
            part = (part + terms[:, :, g]).astype(np.float32)
        acc[sel] = part
    return rows, cols, acc


# ------------------------------------------------------------------------------------------------
# the GPU side: one call of a case's C entry in the lab library, every buffer embedded in allocated surroundings
# ------------------------------------------------------------------------------------------------
def blocked(sf_rows: np.ndarray) -> np.ndarray:
    """to_blocked of ALL the given rows (a multiple of 128: the padding rows keep what the caller put there)"""
    assert sf_rows.shape[0] % 128 == 0
    return oracle.to_blocked(sf_rows)


def past_k_columns(c: Case):
    """row-major (row, column) mask of the blocked image's scale columns past K inside the last 4-column block"""
    kb = c.k // 32
    return np.arange(-(-kb // 4) * 4) >= kb


def operands(c: Case, d: Data, past_k=None):
    """the byte images the op reads: (A, B, A_sf, B_sf).  past_k: an rng -- the scale columns past K of the blocked images get random FINITE bytes instead of zeros"""
    kb = c.k // 32
    a = np.ascontiguousarray(d.a.T) if c.op == "nn" else d.a
    if c.op == "ada" or c.grouped:
        return a, d.b, np.ascontiguousarray(d.sa[:c.m]), np.ascontiguousarray(d.sb[:GROUPED_E * c.n if c.op != "ada" else c.n])

    def img(s):
        cb = -(-kb // 4) * 4
        full = np.zeros((s.shape[0], cb), np.uint8)
        if past_k is not None:
            full[:] = past_k.integers(0, 255, size=full.shape, dtype=np.uint8)
        full[:, :kb] = s
        return blocked(full)
    return a, d.b, img(d.sa), img(d.sb)


class Embedded:
    """`data` inside a device buffer of `fill` bytes: 4 KiB before it, `post` bytes behind it"""

    def __init__(self, data: np.ndarray, fill: int, post: int, dev):
        import torch

        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        host = np.full(4096 + raw.size + post, fill, np.uint8)
        host[4096:4096 + raw.size] = raw
        self.buf = torch.from_numpy(host).to(dev)
        self.ptr = self.buf.data_ptr() + 4096


class Result(NamedTuple):
    out: np.ndarray          # (m, n) bf16 bits
    guards_ok: bool          # both guard bands of D still hold the sentinel in every element
    unwritten: int           # elements of D that still hold the sentinel
    ws_bytes: int
    ws_tail_ok: bool


def _entry(lib, name, argtypes):
    import ctypes

    f = getattr(lib, name)
    f.restype, f.argtypes = ctypes.c_int, argtypes
    return f


def run(c: Case, d: Data, fill: int = 0xFF, past_k=None, dev="cuda:0") -> Result:
    """One call of the case's form.  A, B and the scale operands lie inside buffers of `fill` bytes (a further tile of rows behind each), D is rows
    [GUARD_ROWS, GUARD_ROWS + m) of a sentinel-filled buffer, the workspace is the queried size plus a sentinel tail."""
    import ctypes

    import torch

    import _benchlib as lab

    lib = lab.load()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    a, b, sfa, sfb = operands(c, d, past_k)
    rowbytes = c.k if c.fp8 else c.k // 2
    ea, eb = Embedded(a, fill, 256 * rowbytes, dev), Embedded(b, fill, 256 * (c.k // 2 if c.op == "g48" else rowbytes), dev)
    esa, esb = Embedded(sfa, fill, 1 << 16, dev), Embedded(sfb, fill, 1 << 16, dev)
    alpha = torch.tensor([d.alpha], device=dev)
    dbuf = torch.full((c.m + 2 * GUARD_ROWS, c.n), SENTINEL, dtype=torch.int16, device=dev)
    dptr = dbuf.data_ptr() + GUARD_ROWS * c.n * 2
    stream = torch.cuda.current_stream().cuda_stream
    with lab.forced(gemm_variant=c.variant, **dict(c.opts)):
        if c.op in ("mxf4", "mxf8"):
            ws_bytes = lib.qutlass_amd_gemm_splitk_workspace_bytes(8 if c.fp8 else 4, c.m, c.n, c.k)
        elif c.op == "nn":
            ws_bytes = lib.qutlass_amd_mxf8_nn_workspace_bytes(c.m, c.k)
        else:
            ws_bytes = 0
        ws = torch.full((ws_bytes + WS_TAIL,), 0xA5, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() if ws_bytes else None
        head = (ea.ptr, eb.ptr, esa.ptr, esb.ptr, alpha.data_ptr())
        if c.op == "mxf4":
            rc = lib.qutlass_amd_matmul_mxf4_bf16_tn_ws(*head, dptr, c.m, c.n, c.k, wsp, ws_bytes, stream)
        elif c.op == "ada":
            rc = lib.qutlass_amd_matmul_ada_mxf4_bf16_tn(*head, dptr, c.m, c.n, c.k, stream)
        elif c.op == "mxf8":
            rc = lib.qutlass_amd_matmul_mxf8_bf16_tn_fmt(*head, dptr, c.m, c.n, c.k, int(c.a5), 0, wsp, ws_bytes, stream)
        elif c.op == "nn":
            f = _entry(lib, "qutlass_amd_matmul_mxf8_bf16_nn_fmt", [vp] * 6 + [i64] * 3 + [i32, i32, vp, i64, vp])
            rc = f(*head, dptr, c.m, c.n, c.k, int(c.a5), 0, wsp, ws_bytes, stream)
        else:
            offs = torch.tensor(np.cumsum(group_counts(c)), dtype=torch.int32, device=dev)
            tail = [i64] * 4 + ([i32] if c.op == "g8" else []) + [vp]
            kind = {"g4": "mxf4", "g8": "mxf8", "g48": "mxf8_mxf4"}[c.op]
            f = _entry(lib, f"qutlass_amd_grouped_matmul_{kind}_bf16_tn", [vp] * 5 + [i64, vp, vp] + tail)
            fmt = (int(c.a5),) if c.op == "g8" else ()
            rc = f(*head, 1, offs.data_ptr(), dptr, c.m, c.n, c.k, GROUPED_E, *fmt, stream)
        assert rc == 0, lib.qutlass_amd_last_error().decode()
        torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL, dtype=torch.int16, device=dev)
    guards_ok = bool((dbuf[:GUARD_ROWS] == sent).all()) and bool((dbuf[GUARD_ROWS + c.m:] == sent).all())
    body = dbuf[GUARD_ROWS:GUARD_ROWS + c.m]
    return Result(body.cpu().numpy().view(np.uint16), guards_ok, int((body == sent).sum()), ws_bytes, bool((ws[ws_bytes:] == 0xA5).all()))


def assert_footprint(r: Result):
    assert r.guards_ok, "the guard rows around D were written"
    assert r.unwritten == 0, f"{r.unwritten} elements of D were never written"
    assert r.ws_tail_ok, f"the workspace was written past the {r.ws_bytes} bytes handed over"


def assert_equals_reference(out, ref):
    """isnan(out) == isnan(ref) over the whole output, every other element equal byte for byte (+-inf included)"""
    gn, rn = isnan_bf16(out), isnan_bf16(ref)
    assert np.array_equal(gn, rn), f"NaN pattern: {int((gn & ~rn).sum())} unexpected, {int((rn & ~gn).sum())} missing, first at {np.argwhere(gn != rn)[0].tolist()}"
    bad = (out != ref) & ~rn
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} outputs differ, first at {np.argwhere(bad)[0].tolist()}: got {out[bad][:4]}, oracle {ref[bad][:4]}"
