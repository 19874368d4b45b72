"""The two tables of qutlass_amd/ops.py -- QUANT_OPS (the rotate + quantize family) and OUTPUT_OPS (every other op that fills results it is handed) -- against the op
library: every in-place op is the twin of exactly one row, every row's functional op exists with the row's schema, and what the functional op returns under
FakeTensorMode is what the row's allocator gives -- the one allocator the eager wrappers of qutlass_amd/__init__.py use as well."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import ops

DEV = "cuda"
DIRECT = ()   # in-place ops without a row, called directly by a wrapper: none
ROWS = {**ops.QUANT_OPS, **ops.OUTPUT_OPS}
BF, U8, I32, I64, F32, E8 = torch.bfloat16, torch.uint8, torch.int32, torch.int64, torch.float32, torch.float8_e8m0fnu


def test_the_tables_do_not_overlap():
    assert len(ROWS) == len(ops.QUANT_OPS) + len(ops.OUTPUT_OPS) == 16 + 12
    assert list(ops.OUTPUT_OPS) == ["silu_and_mul", "moe_combine", "swiglu_oai_and_mul", "moe_combine_bias", "moe_topk_softmax", "moe_topk_grouped", "moe_sort_fused",
                                    "quantize_mx_mask", "backward_t", "backward_qt", "square_double_mxfp8", "transpose_mxfp8"]


def test_every_in_place_op_is_the_twin_of_one_row():
    twins = [row.twin for row in ROWS.values()]
    assert len(set(twins)) == len(twins)
    writing = set()
    for schema in torch._C._jit_get_all_schemas():
        if schema.name.startswith("qutlass_amd::") and any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments):
            writing.add(schema.name.split("::")[1])
    assert len(writing) == 28 and writing == set(twins) | set(DIRECT), sorted(writing ^ (set(twins) | set(DIRECT)))
    for name in writing:   # and each has the fake kernel that lets a caller trace it
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{name}").fake_impl.kernel is not None, name


@pytest.mark.parametrize("name", list(ROWS))
def test_the_functional_op_has_the_schema_of_its_row(name):
    schema = getattr(torch.ops.qutlass_amd, name).default._schema
    assert schema == torch._C.parse_schema(f"qutlass_amd::{name}{ROWS[name].schema}"), str(schema)
    assert not any(a.alias_info is not None for a in schema.arguments) and not any(r.alias_info is not None for r in schema.returns), str(schema)


def _t(*shape, dtype=BF):
    return torch.empty(shape, dtype=dtype, device=DEV)


def _quant_args(row):
    """every call of one family op: smallest legal shapes; both values of `blocked` and both code dtypes where they are arguments, with and without the optional tensors"""
    lead = {ops._same: [_t(2, 64)], ops._act: [_t(3, 128)], ops._gathered: [_t(4, 64)]}[row.operand] + [_t(32, 32)]
    by_name = {"src_row": [_t(3, dtype=I32)], "global_scale": [_t(1, dtype=F32)], "global_scales": [_t(2, dtype=F32)], "offs": [_t(2, dtype=I32)], "method": [1],
               "alpha": [1.702], "limit": [7.0], "blocked": [False, True], "dtype": list(ops.MXF8_DTYPES)}
    if row.optional:
        by_name.update(bias=[None, _t(2, 128)], offs=[None, _t(2, dtype=I32)])
    calls = [lead]
    for a in torch._C.parse_schema("x::y" + row.schema).arguments[2:]:
        calls = [c + [v] for c in calls for v in by_name[a.name]]
    return calls


def _output_args():
    h = _t(32, 32)
    return {
        "silu_and_mul": [(_t(3, 96),)],
        "moe_combine": [(_t(4, 8), _t(2, 2, dtype=I32), _t(2, 2, dtype=F32))],
        "swiglu_oai_and_mul": [(_t(3, 96), 1.702, 7.0, None, None), (_t(3, 96), 1.702, 7.0, _t(2, 96), _t(2, dtype=I32))],
        "moe_combine_bias": [(_t(4, 8), _t(2, 2, dtype=I32), _t(2, 2, dtype=F32), _t(1, 8), None), (_t(4, 8), _t(2, 2, dtype=I32), _t(2, 2, dtype=F32), _t(2, 8), _t(2, dtype=I32))],
        "moe_topk_softmax": [(_t(2, 8, dtype=F32), 2, True)],
        "moe_topk_grouped": [(_t(2, 8, dtype=F32), None, 2, 1, 1, 0, True, 1.0, False), (_t(2, 8), _t(8, dtype=F32), 2, 2, 1, 1, False, 2.5, True)],
        "moe_sort_fused": [(_t(2, 2, dtype=I32), None, 8), (_t(2, 2, dtype=I64), _t(8, dtype=I32), 4)],
        "quantize_mx_mask": [(_t(2, 64), h)],
        "backward_t": [(_t(2, 128, 64), h)],
        "backward_qt": [(_t(2, 128, 32, dtype=U8), _t(2, 128, 2, dtype=E8), h, _t(1, dtype=F32))],
        "square_double_mxfp8": [(_t(200, 64),)],      # 200 rows: padded to 256
        "transpose_mxfp8": [(_t(200, 32, dtype=U8), _t(200, 2, dtype=E8))],
    }


def _desc(ts):
    return [(tuple(t.shape), t.dtype, t.device) for t in (ts if isinstance(ts, (tuple, list)) else (ts,))]


@pytest.mark.parametrize("name", list(ROWS))
def test_the_functional_op_returns_what_the_allocator_of_its_row_gives(name):
    row = ROWS[name]
    with FakeTensorMode():
        calls = _quant_args(row) if name in ops.QUANT_OPS else _output_args()[name]
        for args in calls:
            want = ops.alloc_quant(row, *args) if name in ops.QUANT_OPS else row.alloc(*args)
            got = getattr(torch.ops.qutlass_amd, name)(*args)
            assert isinstance(got, torch.Tensor) == isinstance(want, torch.Tensor) and _desc(got) == _desc(want), (name, _desc(got), _desc(want))
            assert all(d[2].type == "cuda" for d in _desc(got))


def test_the_shapes_the_allocators_give():
    """the paddings and transpositions, spelled out once"""
    e4 = torch.float8_e4m3fn
    with FakeTensorMode():
        a = _output_args()
        got = {n: _desc(ops.OUTPUT_OPS[n].alloc(*a[n][-1])) for n in a}
        no_scores = _desc(ops.OUTPUT_OPS["moe_topk_grouped"].alloc(*a["moe_topk_grouped"][0]))
    d = torch.device(DEV, 0)
    assert got["silu_and_mul"] == [((3, 48), BF, d)] and got["swiglu_oai_and_mul"] == got["silu_and_mul"]
    assert got["moe_combine"] == [((2, 8), BF, d)] and got["moe_combine_bias"] == got["moe_combine"]
    assert got["moe_topk_softmax"] == [((2, 2), F32, d), ((2, 2), I32, d)]
    assert got["moe_topk_grouped"] == got["moe_topk_softmax"] + [((2, 8), F32, d)]
    assert got["moe_sort_fused"] == [((4,), I32, d), ((4,), I32, d), ((2, 2), I32, d)]
    assert got["quantize_mx_mask"] == [((2, 32), U8, d), ((128, 4), E8, d), ((2, 8), U8, d)]
    assert got["backward_t"] == [((2, 64, 64), torch.float4_e2m1fn_x2, d), ((2, 64, 4), E8, d)] and got["backward_qt"] == got["backward_t"]
    assert got["square_double_mxfp8"] == [((256, 64), e4, d), ((256, 2), E8, d), ((64, 8), E8, d)]       # rows padded to 128
    assert got["transpose_mxfp8"] == [((64, 256), e4, d), ((64, 8), E8, d)]                               # rows padded to 256
    assert no_scores == got["moe_topk_softmax"] + [((0,), F32, d)]                                        # scores that are not asked for: an empty tensor


def test_the_eager_wrappers_reach_the_runner_of_the_table(monkeypatch):
    """no wrapper allocates: each hands the functional op's arguments to run_output with its row"""
    seen = []
    monkeypatch.setattr(ops, "run_output", lambda row, *a: seen.append((row.twin, len(a))) or (None, None, None))
    m = lambda *s, dtype=BF: torch.empty(*s, dtype=dtype, device="meta")
    h = m(32, 32)
    q.silu_and_mul(m(3, 96))
    q.swiglu_oai_and_mul(m(3, 96))
    q.moe_combine(m(4, 8), m(2, 2, dtype=I32), m(2, 2, dtype=F32))
    q.moe_combine(m(4, 8), m(2, 2, dtype=I32), m(2, 2, dtype=F32), bias=m(1, 8))
    q.moe_topk_softmax(m(2, 8), 2)
    q.moe_topk_grouped(m(2, 8), 2)
    q.moe_sort_fused(m(2, 2, dtype=I32), 8)
    q.fusedQuantizeMx(m(2, 64), h, return_mask=True)
    q.backward_t_bf16(m(2, 128, 64), h)
    q.backward_qt_bf16(m(2, 128, 32, dtype=U8), m(2, 128, 2, dtype=E8), h, m(1, dtype=F32))
    q.backward_bf16_square_double_mxfp8(m(200, 64))
    q.mxfp4_transpose_mxfp8(m(200, 32, dtype=U8), m(200, 2, dtype=E8))
    assert seen == [("siluAndMul_", 1), ("swigluOaiAndMul_", 5), ("moeCombine_", 3), ("moeCombineBias_", 5), ("moeTopkSoftmax_", 3), ("moeTopkGrouped_", 9), ("moeSort_", 3),
                    ("fusedQuantizeMxMask_", 2), ("backward_t_bf16_", 2), ("backward_qt_bf16_", 4), ("backward_bf16_square_double_mxfp8_", 1), ("mxfp4_transpose_mxfp8_", 2)]
