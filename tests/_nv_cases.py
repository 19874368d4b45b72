"""Forms, shapes and operand builders shared by tests/test_nv_scale_range_cpu.py (no GPU) and tests/test_gpu_nv_scale_range.py: the NVFP4 twin of tests/_mx_cases.py.

A CASE is one kernel form of one NVFP4 GEMM op at one shape: (op, variant, lab options, m, n, k).
  op       "nv" matmul_nvf4_bf16_tn (_ws entry, to_blocked scales, the queried workspace) | "gnv" grouped_matmul_nvf4_bf16_tn (row-major scales, m = token rows over
           GROUPED_E experts in _mx_cases.group_counts' pattern, offs[-1] == m)
  variant  "nv": the lab library's "nvf4_variant" (gemm_nvf4.hip.h nvf4_launch_plan decodes it; the `variant` column of NV_FORMS); "gnv": its "gemm_variant" 598 ... 601
  options  deepp_grid: workgroups of the forced persistent kernel (variant 42), so that each walks several tiles

The forms are ONE list, gemm_nvf4.hip.h's enum NvForm with one NV_FORMS row each (tile, kernel family, forcing lab variant): its values are the cfg that
qutlass_amd_debug_nvf4_plan reports and the form that qutlass_amd_debug_nvf4_launch_plan writes.  What the product's plan (nvf4_plan: cfg, K ranges) can return, and the
lab variant that runs the same kernel -- plan_variant() below:
  cfg -1 -> 3 skinny split-K kernel | -2 -> 46, -4 ... -11 -> 48 ... 55 wave-owned forms (-3 = 47, 16 columns, stays lab-only) | 0 -> 42 persistent 256x256
  (K % 256 == 0, K >= 512) or 41 per-tile 256x256 | 4 -> 40 256x128 | 1, 2, 3 -> 5, 6, 7 128x128, 128x64, 64x64 in one pass, or 100 + 10 cfg + S: S K ranges into the
  caller's scratch + splitk_reduce_kernel<S> (the split kernel is one instantiation per tile, the reduce kernel one per S: every tile is run split and every S the
  plan can ask for is run, not every pair).

Shapes are the smallest at which a form can still go wrong: two tiles plus a ragged remainder in M (not a multiple of 16; form 53 takes at most 8 rows) and in N (a
multiple of 8, not of the tile).  A stage is 256 K elements.  Forms whose kernel does not depend on K run K = 2432 (9.5 stages, K % 256 == 128) and K = 2464
(K % 64 == 32: the last 4-column block of the blocked scale image is partly past K); the persistent kernel takes whole stages only (9 and 10).  The wave-owned forms
pick their instantiation by KT = ceil(K / 256) (gemm_nvf4_os.hip.h launch_nvf4_os): every instantiation runs at the largest KT it takes, with a ragged last stage,
the next one at the KT just beyond, and the refilled-slot form at a KT past twice its slots (the ring wraps twice).  The grouped op takes K % 128 == 0 only: its
K are K % 256 == 128, where the upper scale dwords of the last stage would be the next row's.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import oracle
from _mx_cases import (GROUPED_E, GUARD_ROWS, SENTINEL, T32, T64, T128, T256, WS_TAIL, Embedded, Result, _entry, assert_equals_reference, assert_footprint,  # noqa: F401
                       blocked, f32_to_bf16_bits, group_counts, isnan_bf16, nan_pattern, pad128)


class Case(NamedTuple):
    op: str
    variant: int
    opts: tuple
    m: int
    n: int
    k: int

    @property
    def id(self):
        o = "".join(f"-{k}{v}" for k, v in self.opts)
        return f"{self.op}-v{self.variant}{o}-{self.m}x{self.n}x{self.k}"

    @property
    def key(self):
        """forms that share (op, shape) share the operands and the reference"""
        return self._replace(variant=0, opts=())

    @property
    def requested_splits(self):
        return self.variant % 10 if self.op == "nv" and 100 <= self.variant < 140 else 1

    @property
    def splits(self):
        """K ranges a forced split launches (nvf4_launch_plan: an even number of stages per range, none empty)"""
        s, kt = self.requested_splits, stages(self.k)
        per = 2 * (-(-kt // (2 * s)))
        return -(-kt // per) if s > 1 else 1


def stages(k):
    return -(-(k // 2) // 128)


G = ("deepp_grid", 2)
TILE_K = (2432, 2464)
OS16_K = (2016, 4064, 4224, 8736)                # KT = 8 | 16, 17 | 35: one stage per wave, two, two refilled slots per wave (16 slots)
OS8_K = (2016, 2176, 4640)                       # KT = 8 | 9, 19: one slot per wave, refilled beyond (8 slots)
OS32_K = (2016, 4064, 6112, 8160, 8320, 16544)   # KT = 8 | 16 | 24 | 32 | 33, 65: one to four stages per wave, four refilled slots per wave (32 slots)
T12864 = (275, 168)

# (variant, options, (m, n), K list)
_DENSE = [
    (3, (), T32, TILE_K),                        # skinny split-K kernel, 32x32 tiles
    (46, (), T32, OS16_K),                       # wave-owned 32x32
    (48, (), (37, 40), OS32_K),                  # ... its 16x16 decode form
    (49, (), (83, 40), OS16_K),                  # ... 32x16
    (50, (), (37, 72), OS16_K), (51, (), (37, 104), OS16_K),   # ... 16 rows x 32 / 48 columns
    (52, (), (37, 120), OS8_K),                  # ... x 56 columns
    (53, (), (7, 120), OS16_K),                  # ... x 56 columns, A rows 0 ... 7 only
    (54, (), (147, 72), OS8_K), (55, (), (211, 72), OS8_K),    # 64x32 / 96x32 tiles
    (42, (G,), T256, (2304, 2560)),              # persistent 256x256: 9 tiles on 2 workgroups
    (42, (), T256, (2304, 2560)),                # ... one tile per workgroup
    (41, (), T256, TILE_K),                      # per-tile 256x256 (what the product runs when K % 256 != 0)
    (40, (), (531, 296), TILE_K),                # 256x128
    (5, (), T128, TILE_K), (6, (), T12864, TILE_K), (7, (), T64, TILE_K),
    # split-K: every tile with 2 ranges, and one reduce instantiation each for 3 ... 8 (a range is 4 stages or more, as in the plan)
    (112, (), T128, (2432,)), (113, (), T128, (2432,)), (114, (), T128, (4064,)),
    (122, (), T12864, (2432,)), (125, (), T12864, (5088,)), (126, (), T12864, (6112,)),
    (132, (), T64, (2432,)), (137, (), T64, (7136,)), (138, (), T64, (8160,)),
    (138, (), T64, (5088,)),                     # 8 ranges requested, 20 stages: 5 non-empty ranges
]
_GROUPED = [(598, (1920, 3968, 4224, 8576)), (599, (1920, 2176, 4480)), (600, (2432,)), (601, (2432,))]   # 598 / 599: launch_nvf4_grouped's KT rule (16 / 8 slots)
GROUPED_SHAPE = (300, 200)

CASES = [Case("nv", v, o, m, n, k) for v, o, (m, n), ks in _DENSE for k in ks] + [Case("gnv", v, (), *GROUPED_SHAPE, k) for v, ks in _GROUPED for k in ks]
KEYS = sorted({c.key for c in CASES}, key=lambda c: c.id)


def covered(op):
    """the forms of an op that CASES runs; a split form counts as 100 + 10 cfg (its kernel does not depend on the number of ranges)"""
    return {c.variant - c.variant % 10 if c.requested_splits > 1 else c.variant for c in CASES if c.op == op}


def covered_splits():
    """the numbers of K ranges (= the splitk_reduce_kernel instantiations) CASES runs"""
    return {c.splits for c in CASES if c.splits > 1}


def plan_variant(cfg, splits, k):
    """the lab form of what nvf4_plan returned for a shape with this K: (variant as in covered(), K ranges)"""
    if cfg < 0:
        return {-1: 3, -2: 46, -3: 47}.get(cfg, 44 - cfg), 1
    if cfg == 0:
        return (42 if k % 256 == 0 and k >= 512 else 41), 1
    if cfg == 4:
        return 40, 1
    return (100 + 10 * cfg, splits) if splits > 1 else (4 + cfg, 1)


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
FINITE = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)                 # the 254 e4m3 bytes that are not NaN, in byte order
EXTREMES = (0x00, 0x01, 0x07, 0x08, 0x38, 0x7E, 0x80, 0x81, 0x87, 0x88, 0xB8, 0xFE)      # zero, smallest / largest subnormal, smallest normal, 1.0, 448; both signs
QUANTUM = 2.0 ** -5                                                                      # of every term of the whole-range layouts (see _whole_range)
LONG_K = 6000
SMALL_CODES = np.array([0, 1, 2, 3, 4, 8, 9, 10, 11, 12], np.uint8)                      # |value| <= 2


@functools.lru_cache(maxsize=None)
def e4m3_table():
    return np.array([oracle.lib().orc_e4m3_decode(i) for i in range(256)], np.float64)


@functools.lru_cache(maxsize=None)
def e2m1_table():
    return np.array([oracle.lib().orc_e2m1_decode(i) for i in range(16)], np.float64)


def pow2_byte(x):
    """the e4m3 byte of 2^x, x in -9 ... 8"""
    x = np.asarray(x)
    assert x.min() >= -9 and x.max() <= 8
    return np.where(x >= -6, (x + 7) << 3, 1 << np.clip(x + 9, 0, 2)).astype(np.uint8)


def scale_walk(kb, layout):
    """index into FINITE of K group g.  "sweep": 97 g mod 254 walks all the finite bytes in large steps; "extremes": the EXTREMES list in adjacent groups"""
    g = np.arange(kb)
    if layout == "sweep":
        return (97 * g) % 254
    return np.searchsorted(FINITE, np.array(EXTREMES, np.uint8))[g % len(EXTREMES)]


def _whole_range(rows_walk, rows_comp, kb, layout):
    """The walking operand's byte runs over the finite e4m3 range along the K groups, the other operand holds the power of two that brings the group's scale product
    back to 1 ... 4: walker(r, g) = FINITE[w(g) + u(r)], u in {0, 1}; compensator(c, g) = 2^(-floor(log2 |FINITE[w(g)]|) + v(c)), v in {0, 1}, clamped to 2^-9 ... 2^8
    (a zero byte counts as its neighbour 2^-9, which u(r) = 1 turns it into).  The walker's byte is a multiple of 2^(floor - 3) and at most 2^(floor + 1), so every
    scale product is a multiple of 2^-3 (2^-1 where the clamp cut the compensator) and at most 4; a product of two e2m1 values is a multiple of 2^-2, at most 36:
    every term is a multiple of QUANTUM = 2^-5.  A wrong scale row / column changes u / v and with it the output."""
    w = scale_walk(kb, layout)[None, :]
    walker = FINITE[(w + (rows_walk * 7 + rows_walk // 32) % 2) % 254]
    val = np.abs(e4m3_table()[FINITE[w]])
    val = np.where(val == 0, 2.0 ** -9, val)
    x = -np.floor(np.log2(val)).astype(np.int64) + (rows_comp * 5 + rows_comp // 16) % 2
    return walker, pow2_byte(np.clip(x, -9, 8))


class Data(NamedTuple):
    a: np.ndarray        # (m, k/2) packed e2m1
    b: np.ndarray        # (n, k/2); grouped: (E n, k/2)
    sa: np.ndarray       # (pad128(m), k/16) e4m3 bytes, row-major: rows >= m are what the padding rows of the blocked image hold; grouped: (m, k/16)
    sb: np.ndarray       # (pad128(n), k/16); grouped: (E n, k/16)
    alpha: float


def nan_byte_pattern(c: Case, d: Data):
    """row-major masks of the NaN scale bytes of the tracer data (both operands)"""
    return d.sa & 0x7F == 0x7F, d.sb & 0x7F == 0x7F


@functools.lru_cache(maxsize=None)
def _dataset(key: Case, part: str, walk_a: bool) -> Data:
    c = key
    grouped = c.op == "gnv"
    rng = np.random.default_rng(zlib.crc32(repr((c.op, c.m, c.n, c.k, part, walk_a)).encode()))
    kb = c.k // 16
    rows_a, rows_b = (c.m, GROUPED_E * c.n) if grouped else (pad128(c.m), pad128(c.n))
    nb = rows_b if grouped else c.n

    def codes(rows):
        if c.k <= LONG_K:
            return rng.integers(0, 256, size=(rows, c.k // 2), dtype=np.uint8)
        lo, hi = SMALL_CODES[rng.integers(0, len(SMALL_CODES), size=(2, rows, c.k // 2))]   # (long K: small values keep sum |terms| below 2^24 quanta)
        return (lo | (hi << 4)).astype(np.uint8)

    a, b = codes(c.m), codes(nb)
    ra, rb = np.arange(rows_a)[:, None], np.arange(rows_b)[:, None]
    if part in ("sweep", "extremes"):
        if walk_a:
            sa, sb = _whole_range(ra, rb, kb, part)
        else:
            sb, sa = _whole_range(rb, ra, kb, part)
    else:   # the exact regime of tests/test_gpu_round6.py: 2^-1 ... 2^1 x 1.0 ... 1.875
        sa = rng.integers(0x30, 0x48, size=(rows_a, kb), dtype=np.uint8)
        sb = rng.integers(0x30, 0x48, size=(rows_b, kb), dtype=np.uint8)
    if part == "nan":   # both NaN bytes as tracers, continued through the padding rows of the blocked image; _mx_cases.nan_pattern is the predicted isnan(D)
        sa[(ra[:, 0] % 5) == 1, min(1, kb - 1)] = 0x7F
        sa[(ra[:, 0] % 5) == 3, kb - 1] = 0xFF                 # (grouped: the last scale column of a row)
        col = rb[:, 0] % c.n if grouped else rb[:, 0]
        sb[(col % 7 == 2) & (col // 7 % 2 == 0), kb // 2] = 0x7F
        sb[(col % 7 == 2) & (col // 7 % 2 == 1), kb // 2] = 0xFF
    return Data(a, b, np.ascontiguousarray(sa), np.ascontiguousarray(sb), 0.5)


def dataset(c: Case, part: str, walk_a: bool = True) -> Data:
    """part: "sweep" / "extremes" (walk_a: A's scale byte walks and B's compensates, or the reverse), "nan", "plain" """
    return _dataset(c.key, part, bool(walk_a) if part in ("sweep", "extremes") else True)


def segments(c: Case):
    """(expert, first row, end row) of the row ranges that meet one B: the experts of a grouped case, the whole of a dense one"""
    if c.op != "gnv":
        return [(0, 0, c.m)]
    o = np.r_[0, np.cumsum(group_counts(c))]
    return [(e, int(o[e]), int(o[e + 1])) for e in range(GROUPED_E) if o[e + 1] > o[e]]


@functools.lru_cache(maxsize=None)
def _reference(key: Case, part: str, walk_a: bool) -> np.ndarray:
    c, d = key, _dataset(key, part, walk_a)
    ref = np.empty((c.m, c.n), np.uint16)
    for e, r0, r1 in segments(c):
        be, sbe = (d.b[e * c.n:(e + 1) * c.n], d.sb[e * c.n:(e + 1) * c.n]) if c.op == "gnv" else (d.b, d.sb[:c.n])
        ref[r0:r1] = oracle.gemm_blockscaled(oracle.KIND_NVFP4, d.a[r0:r1], be, oracle.to_blocked(d.sa[r0:r1]), oracle.to_blocked(sbe), d.alpha, r1 - r0, c.n, c.k)
    ref.setflags(write=False)
    return ref


def reference(c: Case, part: str, walk_a: bool = True) -> np.ndarray:
    """(m, n) bf16 bits of the oracle (per expert for "gnv"), computed once per (op, shape, part)"""
    return _reference(c.key, part, bool(walk_a) if part in ("sweep", "extremes") else True)


def dequantised(c: Case, d: Data):
    """fp64 (m, k) and (n or E n, k): e2m1 value x e4m3 scale"""
    t2, t4 = e2m1_table(), e4m3_table()
    unpack = lambda x: np.stack([t2[x & 15], t2[x >> 4]], -1).reshape(x.shape[0], -1)
    return unpack(d.a) * np.repeat(t4[d.sa[:c.m]], 16, axis=1), unpack(d.b) * np.repeat(t4[d.sb[:d.b.shape[0]]], 16, axis=1)


def sums_in_fp32(c: Case, d: Data, reverse: bool):
    """sampled outputs (rows, cols, fp32 sums) with the K groups' block sums added one by one in fp32, forward or reversed: equal bits for both orders = the exact regime"""
    ad, bd = dequantised(c, d)
    kb = c.k // 16
    rows = np.unique(np.concatenate([np.r_[r0:min(r0 + 4, r1), max(r1 - 4, r0):r1] for _, r0, r1 in segments(c)]))
    cols = np.unique(np.r_[0:16, c.n - 16:c.n])
    acc = np.zeros((len(rows), len(cols)), np.float32)
    for e, r0, r1 in segments(c):
        sel = (rows >= r0) & (rows < r1)
        blk = np.einsum("rgi,cgi->rcg", ad[rows[sel]].reshape(-1, kb, 16), bd[e * c.n + cols].reshape(len(cols), kb, 16))
        terms = blk.astype(np.float32)
        assert np.array_equal(terms.astype(np.float64), blk)
        s = np.zeros(terms.shape[:2], np.float32)
        for g in (range(kb - 1, -1, -1) if reverse else range(kb)):
            s = (s + terms[:, :, g]).astype(np.float32)
        acc[sel] = s
    return rows, cols, acc


# ------------------------------------------------------------------------------------------------
# the GPU side: one call of a case's C entry, every buffer embedded in allocated surroundings
# ------------------------------------------------------------------------------------------------
def operands(c: Case, d: Data, past_k=None):
    """the byte images the op reads: (A, B, A_sf, B_sf).  past_k: an rng -- the scale columns past K of the blocked images get random FINITE bytes instead of zeros"""
    if c.op == "gnv":
        return d.a, d.b, d.sa, d.sb
    kb = c.k // 16

    def img(s):
        full = np.zeros((s.shape[0], -(-kb // 4) * 4), np.uint8)
        if past_k is not None:
            full[:] = FINITE[past_k.integers(0, len(FINITE), size=full.shape)]
        full[:, :kb] = s
        return blocked(full)
    return d.a, d.b, img(d.sa), img(d.sb)


def run(c: Case, d: Data, fill: int = 0xFF, past_k=None, dev="cuda:0", lib=None, workspace=True) -> Result:
    """One call of the case's form in the lab library (lib: another library, called as it is: the product, whose rule picks the form).  A, B and the scale operands lie
    inside buffers of `fill` bytes (a further tile of rows behind each), D is rows [GUARD_ROWS, GUARD_ROWS + m) of a sentinel-filled buffer, the workspace is the
    queried size plus a sentinel tail (workspace=False: none is handed over)."""
    import contextlib
    import ctypes

    import torch

    import _benchlib as lab

    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    a, b, sfa, sfb = operands(c, d, past_k)
    ea, eb = Embedded(a, fill, 256 * (c.k // 2), dev), Embedded(b, fill, 256 * (c.k // 2), dev)
    esa, esb = Embedded(sfa, fill, 1 << 16, dev), Embedded(sfb, fill, 1 << 16, dev)
    alpha = torch.tensor([d.alpha], device=dev)
    dbuf = torch.full((c.m + 2 * GUARD_ROWS, c.n), SENTINEL, dtype=torch.int16, device=dev)
    dptr = dbuf.data_ptr() + GUARD_ROWS * c.n * 2
    stream = torch.cuda.current_stream().cuda_stream
    if lib is None:
        lib, force = lab.load(), lab.forced(**{"nvf4_variant" if c.op == "nv" else "gemm_variant": c.variant}, **dict(c.opts))
    else:
        force = contextlib.nullcontext()
    with force:
        head = (ea.ptr, eb.ptr, esa.ptr, esb.ptr, alpha.data_ptr())
        if c.op == "nv":
            query = _entry(lib, "qutlass_amd_nvf4_splitk_workspace_bytes", [i64] * 3)
            query.restype = i64
            ws_bytes = query(c.m, c.n, c.k) if workspace else 0
            ws = torch.full((ws_bytes + WS_TAIL,), 0xA5, dtype=torch.uint8, device=dev)
            f = _entry(lib, "qutlass_amd_matmul_nvf4_bf16_tn_ws", [vp] * 6 + [i64] * 3 + [vp, i64, vp])
            rc = f(*head, dptr, c.m, c.n, c.k, ws.data_ptr() if ws_bytes else None, ws_bytes, stream)
        else:
            ws_bytes = 0
            ws = torch.full((WS_TAIL,), 0xA5, dtype=torch.uint8, device=dev)
            offs = torch.tensor(np.cumsum(group_counts(c)), dtype=torch.int32, device=dev)
            f = _entry(lib, "qutlass_amd_grouped_matmul_nvf4_bf16_tn", [vp] * 5 + [i64, vp, vp] + [i64] * 4 + [vp])
            rc = f(*head, 1, offs.data_ptr(), dptr, c.m, c.n, c.k, GROUPED_E, stream)
        assert rc == 0, lib.qutlass_amd_last_error().decode()
        torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL, dtype=torch.int16, device=dev)
    guards_ok = bool((dbuf[:GUARD_ROWS] == sent).all()) and bool((dbuf[GUARD_ROWS + c.m:] == sent).all())
    body = dbuf[GUARD_ROWS:GUARD_ROWS + c.m]
    return Result(body.cpu().numpy().view(np.uint16), guards_ok, int((body == sent).sum()), ws_bytes, bool((ws[ws_bytes:] == 0xA5).all()))
