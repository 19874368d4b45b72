"""The harness of tests/test_gpu_op_footprint.py (tests/_footprint.py) without a GPU: its extent table against the package's own allocator and the header's words,
its checker on planted faults (a footprint test that cannot fail checks nothing), and the arithmetic behind the shapes the GPU file relies on."""
import re

import numpy as np
import pytest
import torch

import _footprint as fp
from qutlass_amd import _lib, ops
from qutlass_amd.utils import padded_scale_shape

ROTS = {"mx": (32, 64, 128), "nv": (16, 32, 64, 128), "mxf8": (32, 64, 128)}


# ---- the extent table ------------------------------------------------------------------------------------------------------------------------------------------
def _args(row, R, rows, blocked):
    """the arguments alloc_quant takes for an operand of (rows, 3 max(R, 32)), as CPU tensors"""
    k = 3 * fp.rp(R)
    h = torch.empty(R, R, dtype=torch.bfloat16)
    if row.operand is ops._gathered:
        lead = [torch.empty(fp.T_TOK, k, dtype=torch.bfloat16), h, torch.empty(rows, dtype=torch.int32)]
    elif row.operand is ops._act:
        lead = [torch.empty(rows, 2 * k, dtype=torch.bfloat16), h]
    else:
        lead = [torch.empty(rows, k, dtype=torch.bfloat16), h]
    return lead, k


@pytest.mark.parametrize("name", list(ops.QUANT_OPS))
def test_extents_agree_with_the_allocator(name):
    row = ops.QUANT_OPS[name]
    group, _ = ops.QUANT_FORMATS[row.fmt]
    for R in ((32, 64) if name == "swiglu_oai_quantize_mxf8" else ROTS[row.fmt]):
        for blocked in ([False, True] if row.blocked is None else [row.blocked]):
            for rows in fp.BLOCKED_ROWS + (fp.M_ROWS,):
                lead, k = _args(row, R, rows, blocked)
                for dtype in (ops.MXF8_DTYPES if row.fmt == "mxf8" and row.dtype is None else (None,)):   # (a row that fixes its code dtype has no such argument)
                    tail = ([dtype] if dtype is not None else []) + [blocked]      # alloc_quant reads the code dtype behind the leading tensors and `blocked` last
                    codes, sf = ops.alloc_quant(row, *lead, *tail)
                    assert codes.dtype == (torch.uint8 if row.fmt != "mxf8" else dtype or row.dtype), (name, codes.dtype)
                    ext = fp.quant_extents(row.fmt, (rows, k), blocked, fp8_codes=row.fmt == "mxf8")
                    assert ext["OUT"] == (codes.numel() * codes.element_size(),) * 2, (name, R, rows)
                    pr, pc = padded_scale_shape(rows, k, group)
                    assert ext["OUT_sf"][0] == sf.numel() == pr * pc, (name, R, rows, blocked)
                    assert ext["OUT_sf"][1] == (pr * pc if blocked else rows * k // group)
                    assert blocked or ext["OUT_sf"][1] < ext["OUT_sf"][0]      # a flat scale buffer always has a caller-owned tail at these shapes
    assert fp.mask_bytes(70 * 96) == 70 * 96 // 8


def test_extent_table_quotes_the_header():
    text = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", open(fp.HEADER).read()))
    for result, _, quote in fp.EXTENT_TABLE:
        assert re.sub(r"\s+", " ", quote) in text, (result, quote)


# ---- the checker can fail ------------------------------------------------------------------------------------------------------------------------------------------
def _layout():
    x = np.arange(3 * 96, dtype=np.uint16)
    return fp.Layout().input("A", x).input("src_row", np.array([4, 0, 4], dtype=np.int32)).output("OUT", 144).output("OUT_sf", 512, 9).scratch("workspace", 4096, 1024)


def _clean_images(lay):
    """what a correct op leaves: the extents written with the same bytes in both runs, everything else as it was"""
    out = []
    for fill in fp.FILLS:
        img = lay.host_image(fill)
        for v in lay.views.values():
            if v.data is None and not v.scratch:
                img[v.offset:v.offset + v.extent] = (np.arange(v.extent) * 7 + 1) % 251
        out.append(img)
    return out


def test_layout_keeps_bands_and_alignment():
    lay = _layout()
    views = sorted(lay.views.values(), key=lambda v: v.offset)
    assert views[0].offset >= fp.BAND and lay.size - (views[-1].offset + views[-1].nbytes) >= fp.BAND
    for a, b in zip(views, views[1:]):
        assert b.offset - (a.offset + a.nbytes) >= fp.BAND
    assert all(v.offset % fp.ALIGN == 0 for v in views) and fp.BAND % fp.ALIGN == 0
    assert fp.BAND == 4 * (4 * 32 * 128)      # four times the span one quantizer workgroup writes: 4 tiles x 32 rows x 128 one-byte codes
    arena = fp.Arena(lay, fp.FILLS[0], "cpu")
    assert arena.t("A", torch.bfloat16, 3, 96).shape == (3, 96) and arena.t("src_row", torch.int32).tolist() == [4, 0, 4]
    assert bool((arena.t("OUT_sf", torch.uint8) == fp.FILLS[0]).all())
    assert arena.ptr("OUT") - arena.buf.data_ptr() == lay.views["OUT"].offset


def test_a_clean_run_passes_and_the_workspace_may_hold_anything():
    lay = _layout()
    images = _clean_images(lay)
    w = lay.views["workspace"]
    images[0][w.offset:w.offset + w.extent] = 1
    images[1][w.offset:w.offset + w.extent] = 2
    assert fp.violations(lay, images) == []
    fp.check(lay, images)


def test_a_byte_one_past_an_extent_is_reported():
    lay = _layout()
    for name, where in (("OUT_sf", 9), ("OUT", 144), ("workspace", 1024)):
        images = _clean_images(lay)
        v = lay.views[name]
        images[1][v.offset + where] = 0x11
        msgs = fp.violations(lay, images)
        assert len(msgs) == 1 and "write outside the extents: 1 bytes in run 1" in msgs[0] and f"first at {name}+{where} " in msgs[0], msgs
        with pytest.raises(AssertionError, match=re.escape(f"{name}+{where}")):
            fp.check(lay, images)
    images = _clean_images(lay)
    images[0][lay.views["OUT"].offset - 3] = 0
    images[0][lay.views["OUT"].offset - 2] = 0
    msgs = fp.violations(lay, images)
    assert len(msgs) == 1 and "2 bytes in run 0" in msgs[0] and "first at OUT-3 " in msgs[0], msgs


def test_a_byte_that_differs_between_the_runs_inside_an_extent_is_reported():
    lay = _layout()
    images = _clean_images(lay)
    v = lay.views["OUT"]
    images[0][v.offset + 17] = fp.FILLS[0]       # a byte the op never wrote: each run still holds its fill
    images[1][v.offset + 17] = fp.FILLS[1]
    msgs = fp.violations(lay, images)
    assert len(msgs) == 1 and "runs differ inside the extent: 1 of 144 bytes of OUT, first at OUT+17" in msgs[0], msgs
    images = _clean_images(lay)                   # a byte written in both runs, but with different values (computed from bytes outside the operands)
    images[1][lay.views["OUT_sf"].offset + 8] ^= 0x40
    msgs = fp.violations(lay, images)
    assert len(msgs) == 1 and "of OUT_sf, first at OUT_sf+8" in msgs[0], msgs


def test_a_changed_input_byte_is_reported():
    lay = _layout()
    images = _clean_images(lay)
    images[1][lay.views["src_row"].offset + 5] ^= 0xFF
    msgs = fp.violations(lay, images)
    assert len(msgs) == 1 and "input changed: 1 bytes of src_row in run 1, first at src_row+5" in msgs[0], msgs


def test_run_twice_on_the_cpu():
    lay = fp.Layout().input("A", np.arange(16, dtype=np.uint8)).output("OUT", 64, 16)
    good = fp.run_twice(lay, lambda a: a.t("OUT", torch.uint8)[:16].copy_(a.t("A", torch.uint8) + 1), "cpu")
    assert good["OUT"].tolist() == list(range(1, 17))
    with pytest.raises(AssertionError, match=r"OUT\+16"):
        fp.run_twice(lay, lambda a: a.t("OUT", torch.uint8)[:17].zero_(), "cpu")                           # one byte too many
    with pytest.raises(AssertionError, match="runs differ inside the extent"):
        fp.run_twice(lay, lambda a: a.t("OUT", torch.uint8)[:15].zero_(), "cpu")                           # one byte too few
    with pytest.raises(AssertionError, match="runs differ inside the extent"):
        fp.run_twice(lay, lambda a: a.t("OUT", torch.uint8)[:16].copy_(a.buf[lay.views["A"].offset + 1:][:16]), "cpu")   # an over-read by one byte


# ---- the shapes give what the GPU file says they give --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_small_shapes_have_a_partial_last_tile_and_idle_waves(cus):
    for R in (16, 32, 64, 128):
        k = 3 * fp.rp(R)
        got = {rows: fp.quant_launch(rows * k, R, cus) for rows in fp.BLOCKED_ROWS + (fp.M_ROWS,)}
        assert [got[r].last_rows for r in fp.ROWS] == [3, 3, 18]          # RP-rows of the last tile
        assert all(0 < g.last_rows < 32 for g in got.values())
        assert got[1].idle_waves == 3 and got[70].idle_waves == 1 and got[fp.M_ROWS].idle_waves == 3 and got[130].idle_waves == 3
        assert all(g.second_trip == 0 for g in got.values())
        for fmt, group in (("mx", 32), ("nv", 16)):
            if k == 96:
                assert (k // group) % 4 != 0                               # scale columns no multiple of 4 (MX 3, NV 6)
    assert padded_scale_shape(130, 96, 32) == (256, 4)                     # two 128-row blocks, 126 padding rows


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_grid_stride_shape_makes_a_second_trip(cus):
    for R in (32, 128):
        rows, k = fp.grid_stride_shape(R, cus)
        assert k == 3 * fp.rp(R) and (rows * k) % fp.rp(R) == 0
        launch = fp.quant_launch(rows * k, R, cus, wg_per_cu=1)
        assert launch.ntiles == 4 * cus + 5 and launch.grid == cus and launch.idle_waves == 0 and launch.second_trip == 5
        assert 0 < launch.last_rows < 32
        if cus == 256:
            assert 7.9 * 2 ** 20 < rows * 3 * 128 * 2 < 8.1 * 2 ** 20      # the largest plain input: about 8 MiB
    assert fp.quant_launch(4096 * 4096, 128, 256).grid == 512              # (the product's own rule: two workgroups per CU at R = 128)


def test_the_65_expert_case_is_not_all_empty():
    c = fp.counts_e65()
    assert len(c) == fp.E65 == 65 and c.sum() == fp.M_ROWS == sum(fp.COUNTS)
    assert int((c == 0).sum()) <= 60
    assert c[64] > 0 and c[:64].sum() > 0                                  # rows on both sides of one wave's width
    assert sum(1 for n in fp.COUNTS if n == 0) == 1 and 1 in fp.COUNTS


def test_sort_sizes_straddle_the_one_launch_bound():
    ws = _lib.load().qutlass_amd_moe_sort_workspace_bytes
    bound = next(n for n in range(8192, 0, -1) if ws(n, 8) == 0)
    assert 63 < bound < 8192 and ws(bound + 1, 8) > 0 and ws(8192, 128) > 0 and ws(8193, 1) > 0
