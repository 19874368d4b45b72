"""The write and read footprint of the ops outside the GEMMs: the harness of tests/test_gpu_op_footprint.py and tests/test_op_footprint_cpu.py.  Plain module: numpy and
torch, no GPU needed to import it or to run the checker.

An ARENA is one uint8 allocation that hands out every operand and every result of one op call as a contiguous view of itself.  Every view has at least BAND = 64 KiB
of band on each side (consecutive views share one): four times the largest span one quantizer workgroup writes, 4 tiles x 32 rows x 128 one-byte codes = 16 KiB, so
a stray store of any tile-sized stride lands in the test's own allocation, where it is seen.  Offsets and bands are multiples of 256 bytes: every pointer keeps the
alignment of a torch allocation (the header wants h 16-byte aligned for R >= 64; misaligned pointers are not what this harness is about).

Every case runs TWICE on identical inputs, the whole arena -- bands, the initial state of every result, the caller-owned tail of a flat scale buffer -- filled with
0x5A the first time and 0xA5 the second.  `check` then asserts, on the two byte images:
  write footprint   inside a result's contractual extent the two runs agree byte for byte (a byte the op never wrote would still hold its run's fill, so no sentinel
                    has to be impossible as an output); every byte outside the extents and outside the inputs still holds its run's fill
  read footprint    the inputs are followed by different bytes in the two runs -- as bf16 a large finite (0x5A5A = 1.5e16) and a negative value (0xA5A5 = -2.9e-16), as
                    int32 two different out-of-range indices, as fp32 two different finite numbers -- so the agreement above also says that no consumed value came
                    from outside an operand; and the inputs themselves are unchanged
The CONTENT of the extents is compared with the op's model by the caller.
"""
from __future__ import annotations

import os
from typing import Callable, NamedTuple

import numpy as np
import torch

BAND = 64 << 10
ALIGN = 256
FILLS = (0x5A, 0xA5)
SORT_WS_TAIL = 1 << 20     # behind moe_sort's workspace: stays untouched

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")


# ------------------------------------------------------------------------------------------------
# the contractual extent of every kind of result, each with the header line it restates (tests/test_op_footprint_cpu.py checks that the quotes are in the header)
# ------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def codes_bytes(numel, fp8=False):
    return numel if fp8 else numel // 2


def flat_scale_bytes(numel, group):
    return numel // group


def blocked_scale_bytes(rows, k, group):
    return ceil_div(rows, 128) * 128 * ceil_div(k // group, 4) * 4


def mask_bytes(numel):
    return numel // 8


EXTENT_TABLE = [
    # (result, extent in bytes, the header's words)
    ("codes (e2m1)", "numel / 2", "out_e2m1: numel/2 bytes"),
    ("codes (fp8)", "numel", "out_fp8: numel bytes, element order"),
    ("flat scales (MX)", "numel / 32, the first bytes of a padded_scale_shape buffer", "out_e8m0: numel/32 bytes written FLAT in group order"),
    ("flat scales (MX), the rest", "caller-owned", "buffer keeps its padding untouched, as in the reference"),
    ("flat scales (NV)", "numel / 16", "out_e4m3: numel/16 bytes (e4m3fn), flat"),
    ("flat scales (gated)", "as the plain op", "blocked == 0 writes the scales flat and leaves the rest of the caller's buffer untouched"),
    ("flat scales (gathering)", "m k / 32 or m k / 16", "bytes of the caller's buffer, the rest untouched"),
    ("flat scales (grouped NV)", "as the sibling", "FLAT row-major scales with the rest"),
    ("flat scales (clamped SwiGLU)", "rows inter / 32", "first rows * inter / 32 bytes, the rest of the caller's buffer untouched"),
    ("flat scales (MXFP8)", "numel / 32", "flat in the first numel / 32 bytes with the rest of the caller's buffer untouched"),
    ("blocked scales", "ceil(rows / 128) 128 ceil(k / group / 4) 4, padding zero", "out_*_blocked: ceil(rows/128)*128 * ceil(k/gs/4)*4 bytes (gs = 32 MX / 16 NV), padding zero-filled"),
    ("clip mask", "numel / 8", "out_mask: NULL, or numel/8 bytes"),
    ("backward_t / backward_qt", "(B, M, N/2) and (B, M, N/32)", "out_e2m1: (B, M, N/2) bytes"),
    ("square_double _rows", "(m_pad, n), (m_pad, n/32), (n, m_pad/32)", "y: (m_pad, n) resp. (n, m_pad); row_scales (m_pad, n/32), col_scales (n, m_pad/32); out_e8m0 (n, m_pad/32)."),
    ("_rows inputs", "m real rows, read-only", "scales are read-only and only need their m real rows"),
    ("sort workspace", "qutlass_amd_moe_sort_workspace_bytes(n, num_experts)", "which must hold qutlass_amd_moe_sort_workspace_bytes(n, num_experts) bytes"),
    ("to_blocked", "ceil(rows / 128) 128 ceil(cols / 4) 4, zero padded", "out: ceil(rows/128)*128 * ceil(cols/4)*4 bytes in the"),
    ("moe_combine", "(t, hdim) bf16", "out (t, hdim) bf16 from y (m, hdim) bf16"),
    ("routing", "(t, topk) float32 / int32, (t, e) float32", "weights (t, topk) float32 and ids (t, topk) int32"),
    ("sort results", "(t topk), (num_experts), (t, topk) int32", "src_row (t * topk), offs (num_experts), pos (t, topk), all int32"),
    ("decode layer", "D (M, N) bf16", "D[M,N] (bf16) = alpha[0] * Q(x . h) (B . SFB)^T"),
]


def quant_extents(fmt: str, shape, blocked: bool, fp8_codes: bool = False):
    """-> {"OUT": (bytes handed over, contractual extent), "OUT_sf": (...)} of one rotate-and-quantize op on an operand of `shape` (.., K); fmt a key of
    qutlass_amd.ops.QUANT_FORMATS.  The scale buffer handed over is always the padded one (padded_scale_shape); flat scales fill its first numel / group bytes."""
    group = {"mx": 32, "nv": 16, "mxf8": 32}[fmt]
    k = shape[-1]
    numel = int(np.prod(shape))
    rows = numel // k
    padded = blocked_scale_bytes(rows, k, group)
    return {"OUT": (codes_bytes(numel, fp8_codes),) * 2, "OUT_sf": (padded, padded if blocked else flat_scale_bytes(numel, group))}


# ------------------------------------------------------------------------------------------------
# the shapes, and what the quantizer's launch makes of them (capi.hip: quant_fill, quant_grid)
# ------------------------------------------------------------------------------------------------
ROWS = (1, 33, 70)             # with K (or I) = 3 max(R, 32): the suite's ragged set
BLOCKED_ROWS = ROWS + (130,)   # two 128-row blocks, 126 padding rows
T_TOK, M_ROWS = 37, 53         # the gathering forms: 53 rows (with repeats) out of 37 tokens
COUNTS = [20, 0, 1, 25, 7]     # rows per expert of the per-expert-scale and bias forms: an empty group, a one-row group, boundaries off the 32-row tiles
E65 = 65                       # ... and a second case whose offs no longer fit one wave's width


def counts_e65():
    """53 rows over 65 experts, most of them empty, rows on both sides of expert 64"""
    c = np.zeros(E65, dtype=np.int64)
    for e, n in ((2, 20), (31, 1), (33, 18), (63, 7), (64, 7)):
        c[e] = n
    return c


def rp(R):
    return max(R, 32)


class QuantLaunch(NamedTuple):
    ntiles: int        # tiles of 32 RP-rows
    last_rows: int     # RP-rows of the last tile (32: a full one)
    grid: int          # workgroups of 4 waves, one tile per wave per trip
    idle_waves: int    # waves of the grid that own no tile at all
    second_trip: int   # waves that walk a second tile


def quant_launch(numel: int, R: int, cus: int, wg_per_cu: int = 0) -> QuantLaunch:
    nrows = numel // rp(R)
    ntiles = ceil_div(nrows, 32)
    per_cu = wg_per_cu if wg_per_cu > 0 else (2 if R >= 128 else 4 if R >= 64 else 8)
    grid = max(1, min(ceil_div(ntiles, 4), cus * per_cu))
    waves = 4 * grid
    return QuantLaunch(ntiles, nrows - 32 * (ntiles - 1), grid, max(0, waves - ntiles), max(0, min(waves, ntiles - waves)))


def grid_stride_shape(R: int, cus: int):
    """(rows, k) with k = 3 max(R, 32) such that ntiles == 4 cus + 5 and the last tile is partial: under quant_wg_per_cu = 1 the grid is `cus` workgroups, every
    wave walks one tile and five of them a second one"""
    ntiles = 4 * cus + 5
    r = next(r for r in range(1, 32) if (32 * (ntiles - 1) + r) % 3 == 0)
    return (32 * (ntiles - 1) + r) // 3, 3 * rp(R)


# ------------------------------------------------------------------------------------------------
# layout, arena, checker
# ------------------------------------------------------------------------------------------------
class View(NamedTuple):
    name: str
    offset: int
    nbytes: int                 # what the op is handed
    extent: int                 # a result: the bytes the contract says are written, from the start of the view; an input: nbytes
    data: np.ndarray | None     # an input: its bytes
    scratch: bool = False       # a workspace: its first `extent` bytes may hold anything afterwards ("contents ... are not kept"), the rest keeps the fill


class Layout:
    """where the operands and results of one call lie in the arena; pure arithmetic"""

    def __init__(self):
        self.views: dict[str, View] = {}
        self._cursor = BAND

    def _place(self, name, nbytes, extent, data, scratch=False):
        assert name not in self.views and nbytes > 0 and 0 <= extent <= nbytes, (name, nbytes, extent)
        self.views[name] = View(name, self._cursor, nbytes, extent, data, scratch)
        self._cursor = ceil_div(self._cursor + nbytes, ALIGN) * ALIGN + BAND

    def input(self, name: str, array) -> "Layout":
        if isinstance(array, torch.Tensor):
            array = array.detach().cpu().contiguous().view(torch.uint8).numpy()
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()
        self._place(name, raw.size, raw.size, raw)
        return self

    def output(self, name: str, nbytes: int, extent: int | None = None) -> "Layout":
        self._place(name, int(nbytes), int(nbytes if extent is None else extent), None)
        return self

    def scratch(self, name: str, nbytes: int, extent: int) -> "Layout":
        self._place(name, int(nbytes), int(extent), None, scratch=True)
        return self

    @property
    def size(self) -> int:
        return self._cursor

    def host_image(self, fill: int) -> np.ndarray:
        img = np.full(self.size, fill, dtype=np.uint8)
        for v in self.views.values():
            if v.data is not None:
                img[v.offset:v.offset + v.nbytes] = v.data
        return img


class Arena:
    def __init__(self, layout: Layout, fill: int, device):
        self.layout = layout
        self.buf = torch.from_numpy(layout.host_image(fill)).to(device)
        assert self.buf.data_ptr() % ALIGN == 0 or self.buf.device.type == "cpu"

    def t(self, name: str, dtype, *shape) -> torch.Tensor:
        """the view `name` as a contiguous tensor of `dtype` (shape: default flat)"""
        v = self.layout.views[name]
        flat = self.buf[v.offset:v.offset + v.nbytes].view(dtype)
        return flat.view(*shape) if shape else flat

    def ptr(self, name: str) -> int:
        return self.buf.data_ptr() + self.layout.views[name].offset

    def image(self) -> np.ndarray:
        return self.buf.cpu().numpy()


def _where(layout: Layout, off: int) -> str:
    """`off` relative to the nearest view: 'OUT_sf+12' (12 bytes behind the view's first byte), 'OUT-3' (3 bytes in front of it)"""
    def dist(v):
        return 0 if v.offset <= off < v.offset + v.nbytes else min(abs(off - v.offset), abs(off - (v.offset + v.nbytes - 1)))
    v = min(layout.views.values(), key=dist)
    return f"{v.name}{off - v.offset:+d}"


def violations(layout: Layout, images) -> list[str]:
    """every way the two runs' byte images break the footprint contract, as messages naming the view, the offset of the first offending byte relative to it, and the
    count"""
    a, b = images
    assert a.shape == b.shape == (layout.size,)
    out = []
    free = np.ones(layout.size, dtype=bool)      # bytes that must still hold the fill
    for v in layout.views.values():
        lo = v.offset
        if v.data is not None:
            free[lo:lo + v.nbytes] = False
            for run, img in enumerate(images):
                bad = np.flatnonzero(img[lo:lo + v.nbytes] != v.data)
                if bad.size:
                    out.append(f"input changed: {bad.size} bytes of {v.name} in run {run}, first at {v.name}+{int(bad[0])}")
        else:
            free[lo:lo + v.extent] = False
            bad = np.flatnonzero(a[lo:lo + v.extent] != b[lo:lo + v.extent])
            if bad.size and not v.scratch:
                out.append(f"runs differ inside the extent: {bad.size} of {v.extent} bytes of {v.name}, first at {v.name}+{int(bad[0])} "
                           f"(0x{int(a[lo + bad[0]]):02x} / 0x{int(b[lo + bad[0]]):02x}): never written, or computed from bytes outside the operands")
    for run, (img, fill) in enumerate(zip(images, FILLS)):
        bad = np.flatnonzero((img != fill) & free)
        if bad.size:
            out.append(f"write outside the extents: {bad.size} bytes in run {run}, first at {_where(layout, int(bad[0]))} (0x{int(img[bad[0]]):02x} over fill 0x{fill:02x})")
    return out


def check(layout: Layout, images) -> None:
    v = violations(layout, images)
    assert not v, "; ".join(v)


def run_twice(layout: Layout, call: Callable[[Arena], None], device="cuda:0") -> dict[str, np.ndarray]:
    """call(arena) once per fill on identical inputs; assert the footprint; -> the extents of the results (bytes of the first run -- the second run's are equal)"""
    images = []
    for fill in FILLS:
        arena = Arena(layout, fill, device)
        call(arena)
        if arena.buf.device.type == "cuda":
            torch.cuda.synchronize()
        images.append(arena.image())
    check(layout, images)
    return {v.name: images[0][v.offset:v.offset + v.extent] for v in layout.views.values() if v.data is None and not v.scratch}


# ------------------------------------------------------------------------------------------------
# the C ABI through ctypes: the ops that allocate their own output, and everything forced through the lab library
# ------------------------------------------------------------------------------------------------
def cabi(lab: bool = False):
    """libqutlass_amd.so, or the lab build of the same sources, with every entry of include/qutlass_amd.h declared (qutlass_amd/_lib.py SYMBOLS)"""
    from qutlass_amd import _lib

    if not lab:
        return _lib.load()
    import _benchlib

    lib = _benchlib.load()
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def ok(lib, rc: int) -> None:
    assert rc == 0, lib.qutlass_amd_last_error().decode()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream
