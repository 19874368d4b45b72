"""The grouped router (moe_topk_grouped, moe_route_grouped) without a GPU: the exported symbol and the header, every argument check of the C entry point (all of
them happen before any HIP call, so dummy pointers are enough), the shape-only kernels of the torch ops, tracing of a layer that starts at moe_route_grouped, the
wrappers' own errors -- and `grouped_topk_ref`, a pure-numpy statement of the op's definition that takes the SCORES as given (so it is exact: float32 s + bias,
float32 top-2 sums, stable sorts), pinned here by hand-written rows and imported by the GPU half, tests/test_gpu_moe_route_grouped.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib

DEV = "cuda"
OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
NAME = "qutlass_amd_moe_topk_grouped"
SIGMOID, SOFTMAX = 0, 1


# ---- the definition, in numpy ---------------------------------------------------------------------------------------------------------
def grouped_topk_ref(s, topk, n_group=1, topk_group=1, bias=None, renormalize=True, routed_scaling_factor=1.0):
    """s (T, E) float32 scores as given -> (ids (T, topk) int64, weights (T, topk) float64, or float32 without renormalize), by the definition:
    c = fl32(s + bias) or s; a group's score is the fl32 sum of its two largest c with a bias (one expert: that value), its largest c without; the first topk_group
    groups in (score descending, index ascending) survive and only their experts are candidates; ids = the first topk candidates in (c descending, index
    ascending), -0 tying with +0 (numpy compares floats); weights = s[ids], float32 times float32(scale) without renormalize (exact), the float64 quotient times
    the scale with it (the kernel's sum order is free, so that is a value to be near, not to equal).  Rows must be free of NaN."""
    s = np.asarray(s, dtype=np.float32)
    T, E = s.shape
    assert E % n_group == 0 and not np.isnan(s).any()
    c = s if bias is None else (s + np.asarray(bias, dtype=np.float32)).astype(np.float32)
    cand = np.ones((T, E), dtype=bool)
    if n_group > 1:
        S = E // n_group
        cg = c.reshape(T, n_group, S)
        if bias is not None and S >= 2:
            top2 = -np.sort(-cg, axis=2)[:, :, :2]                                   # the two largest, as a multiset
            gscore = (top2[:, :, 0] + top2[:, :, 1]).astype(np.float32)             # one float32 add: commutative
        else:
            gscore = cg.max(axis=2)
        assert not np.isnan(gscore).any()
        keep = np.argsort(-gscore, axis=1, kind="stable")[:, :topk_group]             # score descending, group index ascending
        alive = np.zeros((T, n_group), dtype=bool)
        np.put_along_axis(alive, keep, True, axis=1)
        cand = np.repeat(alive, S, axis=1)
    ids = np.empty((T, topk), dtype=np.int64)
    for t in range(T):
        idx = np.flatnonzero(cand[t])                                                 # ascending expert index
        ids[t] = idx[np.argsort(-c[t, idx], kind="stable")[:topk]]                    # c descending, stable: index ascending among equals
    w = np.take_along_axis(s, ids, axis=1)
    if renormalize:
        w64 = w.astype(np.float64)
        return ids, w64 / w64.sum(axis=1, keepdims=True) * float(np.float32(routed_scaling_factor))
    return ids, (w * np.float32(routed_scaling_factor)).astype(np.float32)


def _ref_ids(s, topk, **kw):
    return grouped_topk_ref(np.asarray(s, dtype=np.float32).reshape(1, -1), topk, renormalize=False, **kw)[0][0].tolist()


def test_reference_a_bias_flips_the_choice_but_not_the_weight():
    s = np.array([[0.9, 0.5, 0.1, 0.2]], dtype=np.float32)
    assert _ref_ids(s, 1) == [0]
    bias = np.array([0.0, 0.0, 1.0, 0.0], dtype=np.float32)
    ids, w = grouped_topk_ref(s, 2, bias=bias, renormalize=False, routed_scaling_factor=2.5)
    assert ids[0].tolist() == [2, 0]                                                  # c = 0.9, 0.5, 1.1, 0.2
    assert w.dtype == np.float32 and np.array_equal(w[0], np.array([0.1, 0.9], dtype=np.float32) * np.float32(2.5))   # s, not c
    ids, w = grouped_topk_ref(s, 2, bias=bias, renormalize=True)
    assert np.allclose(w[0], [0.1, 0.9]) and abs(w.sum() - 1.0) < 1e-12


def test_reference_a_masked_groups_largest_expert_is_not_taken():
    # two groups of three; without a bias a group scores its maximum: group 0 (0.8) beats group 1 (0.7); topk = 3 stays inside group 0 although 0.7 > 0.1
    s = [0.8, 0.1, 0.05, 0.7, 0.6, 0.5]
    assert _ref_ids(s, 3, n_group=2, topk_group=1) == [0, 1, 2]
    # the expert with the largest c of ALL sits in the group that loses on the top-2 sum: it is not a candidate
    s = [0.9, 0.0, 0.0, 0.6, 0.6, 0.1]
    zero = np.zeros(6, dtype=np.float32)
    assert _ref_ids(s, 2, n_group=2, topk_group=1, bias=zero) == [3, 4]


def test_reference_a_negative_c_inside_a_surviving_group_beats_everything_outside():
    # bias pushes group 0's c below zero, except one large value that makes group 0 win on its top-2 sum; outside, c is positive but masked
    s = np.array([0.9, 0.2, 0.1, 0.4, 0.3, 0.2], dtype=np.float32)
    bias = np.array([2.0, -1.0, -1.0, 0.0, 0.0, 0.0], dtype=np.float32)              # c = 2.9, -0.8, -0.9 | 0.4, 0.3, 0.2; group scores 2.1 and 0.7
    assert _ref_ids(s, 3, n_group=2, topk_group=1, bias=bias) == [0, 1, 2]            # a zero fill would have taken 3 and 4 (0 > -0.8): this is the -inf mask
    ids, w = grouped_topk_ref(s.reshape(1, -1), 3, n_group=2, topk_group=1, bias=bias, renormalize=False)
    assert np.array_equal(w[0], s[[0, 1, 2]])


def test_reference_ties_go_to_the_lower_group_and_the_lower_expert():
    s = [0.5] * 8
    assert _ref_ids(s, 2, n_group=4, topk_group=2) == [0, 1]                          # groups 0 and 1 of four equal groups, then experts 0 and 1
    assert _ref_ids(s, 3, n_group=4, topk_group=2, bias=np.zeros(8, dtype=np.float32)) == [0, 1, 2]
    s = [0.25, 0.5, 0.5, 0.25, 0.5, 0.25, 0.5, 0.5]                                   # maxima tie everywhere: groups 0, 1; experts 1, 2 before 0, 3
    assert _ref_ids(s, 4, n_group=4, topk_group=2) == [1, 2, 0, 3]
    assert _ref_ids([0.0, -0.0, 0.0, -0.0], 3, bias=np.array([-0.0] * 4, dtype=np.float32)) == [0, 1, 2]   # -0 ties with +0


def test_reference_the_top2_sum_and_the_maximum_disagree():
    s = [0.9, 0.0, 0.0, 0.6, 0.6, 0.0]                                                # group 0: max 0.9, top-2 sum 0.9; group 1: max 0.6, sum 1.2
    assert _ref_ids(s, 1, n_group=2, topk_group=1) == [0]                             # no bias: the maximum decides
    assert _ref_ids(s, 1, n_group=2, topk_group=1, bias=np.zeros(6, dtype=np.float32)) == [3]   # a bias, even all zero: the top-2 sum decides
    # the top two are a multiset: a doubled maximum counts twice
    assert _ref_ids([0.5, 0.5, 0.0, 0.7, 0.2, 0.0], 1, n_group=2, topk_group=1, bias=np.zeros(6, dtype=np.float32)) == [0]
    # groups of one expert score that one value
    assert _ref_ids([0.1, 0.4, 0.3, 0.2], 2, n_group=4, topk_group=2, bias=np.zeros(4, dtype=np.float32)) == [1, 2]
    # a bias of -inf: taken last
    assert _ref_ids([0.9, 0.1, 0.2], 3, bias=np.array([-np.inf, 0, 0], dtype=np.float32)) == [2, 1, 0]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def test_the_symbol_is_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    assert hasattr(lib, NAME) and NAME in _lib.SYMBOLS and f"{NAME}(" in header
    assert "QAMD_MOE_SCORING_SIGMOID 0" in header and "QAMD_MOE_SCORING_SOFTMAX 1" in header and _lib.MOE_SCORING == {"sigmoid": 0, "softmax": 1}


def _tg(t, e, topk, n_group=1, topk_group=1, eb=2, scoring=SIGMOID, bias=None, renorm=1, scale=1.0, logits=X, w=X, ids=X, scores=None):
    return _lib.load().qutlass_amd_moe_topk_grouped(logits, eb, t, e, topk, n_group, topk_group, scoring, bias, renorm, scale, w, ids, scores, None)


def test_topk_grouped_argument_checks():
    assert _tg(0, 8, 2) == OK                                                         # T == 0: nothing to do
    assert _tg(0, 8, 2, logits=None, w=None, ids=None) == OK
    for eb in (0, 1, 3, 8):
        assert _tg(4, 8, 2, eb=eb) == INVALID and "elem_bytes" in _err()
    assert _tg(-1, 8, 2) == INVALID and "bad shape" in _err()
    assert _tg(1 << 31, 8, 2) == INVALID and "bad shape" in _err()
    for e in (0, -1, 1025):
        assert _tg(4, e, 1) == INVALID and "number of experts" in _err()
    for g in (0, -1, 65, 128):
        assert _tg(4, 1024, 1, n_group=g, topk_group=1) == INVALID and "n_group must be in [1, 64]" in _err(), g
    for e, g in ((8, 3), (60, 8), (160, 64), (7, 2)):
        assert _tg(4, e, 1, n_group=g) == INVALID and "n_group must divide E" in _err(), (e, g)
    for g, tg in ((4, 0), (4, -1), (4, 5), (1, 2)):
        assert _tg(4, 8, 1, n_group=g, topk_group=tg) == INVALID and "topk_group" in _err() and "topk must be" not in _err(), (g, tg)
    msg = "topk must be in [1, min(32, topk_group * E / n_group)]"
    for e, topk, g, tg in ((8, 0, 1, 1), (8, -1, 1, 1), (8, 9, 1, 1), (8, 3, 4, 1), (8, 5, 4, 2), (64, 33, 1, 1), (1024, 33, 8, 8), (16, 2, 16, 1), (160, 21, 8, 1)):
        assert _tg(4, e, topk, n_group=g, topk_group=tg) == INVALID and msg in _err(), (e, topk, g, tg)
    for sc in (-1, 2, 7):
        assert _tg(4, 8, 2, scoring=sc) == INVALID and "scoring" in _err()
    assert _tg(4, 8, 2, logits=X + 1) == INVALID and "aligned" in _err()
    assert _tg(4, 8, 2, eb=4, logits=X + 2) == INVALID and "aligned" in _err()
    for arg in ("w", "ids", "bias", "scores"):
        assert _tg(4, 8, 2, **{arg: X + 2}) == INVALID and "aligned" in _err(), arg
    for null in ("logits", "w", "ids"):
        assert _tg(4, 8, 2, **{null: None}) == INVALID and "null pointer" in _err(), null
    # the order of the checks: a bad element size is named even when everything else is wrong too, and nothing was launched for any of the above
    assert _tg(4, 0, 0, n_group=0, topk_group=0, eb=3, scoring=9, logits=None) == INVALID and "elem_bytes" in _err()


# ---- shapes under fake tensors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ops_give_the_right_shapes_under_fake_tensors(dtype):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    T, E, topk = 33, 160, 6
    with FakeTensorMode():
        logits = torch.empty(T, E, dtype=dtype, device=DEV)
        bias = torch.empty(E, dtype=torch.float32, device=DEV)
        two = (q.moe_topk_grouped(logits, topk), q.moe_topk_grouped(logits, topk, n_group=8, topk_group=3, scoring="softmax", renormalize=False),
               q.moe_topk_grouped(logits, topk, n_group=8, topk_group=4, bias=bias, routed_scaling_factor=2.5))
        for res in two:
            assert len(res) == 2
            w, ids = res
            assert w.shape == ids.shape == (T, topk) and w.dtype == torch.float32 and ids.dtype == torch.int32 and w.device.type == ids.device.type == "cuda"
        three = (q.moe_topk_grouped(logits, topk, n_group=8, topk_group=4, bias=bias, return_scores=True), amd.moe_topk_grouped(logits, bias, topk, 8, 4, 0, True, 2.5, True))
        for res in three:
            assert len(res) == 3
            w, ids, s = res
            assert w.shape == ids.shape == (T, topk) and s.shape == (T, E) and s.dtype == w.dtype == torch.float32 and ids.dtype == torch.int32 and s.device.type == "cuda"
        assert amd.moe_topk_grouped(logits, None, topk, 1, 1, 1, True, 1.0, False)[2].numel() == 0            # scores not asked for: an empty third result
        r = q.moe_route_grouped(logits, topk, n_group=8, topk_group=4, bias=bias)
        assert [tuple(a.shape) for a in r] == [(T, topk), (T, topk), (T * topk,), (E,), (T, topk)]
        assert [a.dtype for a in r] == [torch.float32] + [torch.int32] * 4
        emap = torch.empty(E, dtype=torch.int32, device=DEV)
        assert q.moe_route_grouped(logits, topk, 8, n_group=8, topk_group=4, expert_map=emap)[3].shape == (8,)
        want = q.moe_route(logits, topk)
        assert [(a.shape, a.dtype) for a in r] == [(a.shape, a.dtype) for a in want]
        assert q.moe_topk_grouped(torch.empty(0, E, dtype=dtype, device=DEV), topk, return_scores=True)[2].shape == (0, E)


def test_the_in_place_twin_declares_its_writes():
    q.ops.register_torch_ops()
    schema = torch.ops.qutlass_amd.moeTopkGrouped_.default._schema
    written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert written == ["weights", "ids", "scores"] and len(schema.returns) == 0, str(schema)
    assert torch._library.simple_registry.singleton.find("qutlass_amd::moeTopkGrouped_").fake_impl.kernel is not None
    schema = torch.ops.qutlass_amd.moe_topk_grouped.default._schema
    assert not any(a.alias_info is not None for a in schema.arguments) and len(schema.returns) == 3, str(schema)


def test_a_layer_that_starts_at_moe_route_grouped_traces_with_fullgraph():
    E, H, I, T, topk = 8, 256, 128, 35, 2

    def layer(x, logits, bias, h, w13q, w13s, w2q, w2s, alpha):
        topk_w, _, src_row, offs, pos = q.moe_route_grouped(logits, topk, n_group=4, topk_group=2, bias=bias, routed_scaling_factor=2.5)
        aq, asf = q.fusedGatherQuantizeMx(x, h, src_row, method="abs_max")
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        y = q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs)
        return q.moe_combine(y, pos, topk_w)

    with FakeTensorMode():
        args = (torch.empty(T, H, dtype=torch.bfloat16, device=DEV), torch.empty(T, E, dtype=torch.bfloat16, device=DEV), torch.empty(E, device=DEV),
                torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(E, 2 * I, H // 2, dtype=torch.uint8, device=DEV), torch.empty(E * 2 * I * H // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(E, H, I // 2, dtype=torch.uint8, device=DEV), torch.empty(E * H * I // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(1, device=DEV))
        out = torch.compile(layer, backend="eager", fullgraph=True)(*args)
        assert out.shape == (T, H) and out.dtype == torch.bfloat16
        emap = torch.empty(16, dtype=torch.int32, device=DEV)
        r = torch.compile(lambda lg, m: q.moe_route_grouped(lg, topk, 2, scoring="softmax", renormalize=False, expert_map=m), backend="eager", fullgraph=True)(args[1], emap)
        assert [tuple(a.shape) for a in r] == [(T, topk), (T, topk), (T * topk,), (2,), (T, topk)]
        s3 = torch.compile(lambda lg, b: q.moe_topk_grouped(lg, topk, n_group=2, topk_group=1, bias=b, return_scores=True), backend="eager", fullgraph=True)(args[1], args[2])
        assert len(s3) == 3 and s3[2].shape == (T, E)


def test_wrappers_raise_value_error():
    logits = torch.zeros(4, 8)
    for fn in (q.moe_topk_grouped, q.moe_route_grouped):
        for kw in (dict(topk=9), dict(topk=0), dict(topk=3, n_group=4, topk_group=1), dict(topk=5, n_group=4, topk_group=2)):
            with pytest.raises(ValueError, match="topk must be in"):
                fn(logits, **kw)
        with pytest.raises(ValueError, match="topk must be in"):
            fn(torch.zeros(4, 64), 33)
        with pytest.raises(ValueError, match="logits must be"):
            fn(torch.zeros(8), 2)
        with pytest.raises(ValueError, match="n_group must divide E"):
            fn(logits, 1, n_group=3)
        for g in (0, 65):
            with pytest.raises(ValueError, match="n_group must be in"):
                fn(torch.zeros(4, 130), 1, n_group=g)
        for tg in (0, 5):
            with pytest.raises(ValueError, match="topk_group must be in"):
                fn(logits, 1, n_group=4, topk_group=tg)
        with pytest.raises(ValueError, match="scoring must be"):
            fn(logits, 2, scoring="relu")
        with pytest.raises(ValueError, match="number of experts"):
            fn(torch.zeros(2, 1025), 2)
        for bias in (torch.zeros(7), torch.zeros(8, 1), torch.zeros(8, dtype=torch.bfloat16), torch.zeros(0)):
            with pytest.raises(ValueError, match="bias must be"):
                fn(logits, 2, bias=bias)


def test_alias_package_exposes_the_new_functions():
    import qutlass

    for n in ("moe_topk_grouped", "moe_route_grouped"):
        assert getattr(qutlass, n) is getattr(q, n)
