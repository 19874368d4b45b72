"""The one-launch routing (moe_route_fused, moe_route_grouped_fused) without a GPU: the exported symbols and the header, every argument check of the two C entries
(all of them happen before any HIP call, so dummy pointers are enough), the bound query, the launch plan through the debug function, the shape-only kernels of the
two functional ops under FakeTensorMode, make_fx, the schemas, and the Python wrappers' own errors.  The GPU half is tests/test_gpu_moe_route_fused.py."""
import ctypes
import os

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib

DEV = "cuda"
OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
NAMES = ("qutlass_amd_moe_route_fused", "qutlass_amd_moe_route_grouped_fused", "qutlass_amd_moe_route_fused_max_tokens")
F32, I32 = torch.float32, torch.int32


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def _bound():
    return _lib.load().qutlass_amd_moe_route_fused_max_tokens()


def test_the_three_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
        assert f"{name}(" in header, name


def test_the_bound_is_at_most_the_kernels_limit():
    assert 0 <= _bound() <= 64


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def _soft(t=4, e=8, topk=2, eb=2, logits=X, w=X, ids=X, ne=8, emap=None, g=0, src=X, offs=X, pos=X, ng=1):   # (ng: the grouped entry's, ignored)
    return _lib.load().qutlass_amd_moe_route_fused(logits, eb, t, e, topk, 1, w, ids, ne, emap, g, src, offs, pos, None)


def _grp(t=4, e=8, topk=2, ng=2, tg=1, scoring=0, bias=None, eb=2, logits=X, w=X, ids=X, ne=8, emap=None, g=0, src=X, offs=X, pos=X):
    return _lib.load().qutlass_amd_moe_route_grouped_fused(logits, eb, t, e, topk, ng, tg, scoring, bias, 1, 2.5, w, ids, ne, emap, g, src, offs, pos, None)


@pytest.mark.parametrize("entry", [_soft, _grp], ids=["softmax", "grouped"])
def test_argument_checks_shared_by_both_entries(entry):
    assert entry(t=0) == OK                                                     # T == 0: nothing to do, nothing dereferenced
    assert entry(t=0, logits=None, w=None, ids=None, src=None, offs=None, pos=None) == OK
    assert entry(t=65) == INVALID and "at most 64 tokens" in _err() and "65" in _err()
    assert entry(t=-1) == INVALID and "bad shape" in _err()
    for eb in (0, 1, 3, 8):
        assert entry(eb=eb) == INVALID and "elem_bytes" in _err()
    for e in (0, 1025):
        assert entry(e=e, topk=1, ng=1) == INVALID and "number of experts must be in [1, 1024]" in _err(), e
    for ne in (0, 1025):
        assert entry(ne=ne) == INVALID and "number of experts must be in [1, 1024]" in _err(), ne
    assert entry(emap=X, g=0) == INVALID and "expert_map of 0 entries" in _err()   # a map has at least one entry
    assert entry(emap=X, g=-1) == INVALID and "expert_map" in _err()
    for null in ("logits", "w", "ids", "src", "offs", "pos"):
        assert entry(**{null: None}) == INVALID and "null pointer" in _err(), null
    assert entry(logits=X + 1) == INVALID and "aligned" in _err()
    for off in ("w", "ids", "src", "offs", "pos"):
        assert entry(**{off: X + 2}) == INVALID and "aligned" in _err(), off
    assert entry(emap=X + 2, g=4) == INVALID and "aligned" in _err()


def test_softmax_entry_topk_checks():
    for e, topk in ((8, 0), (64, 33), (8, 9), (1, 2), (1024, 33)):              # 0, 33 and E + 1
        assert _soft(e=e, topk=topk) == INVALID and "topk must be in [1, min(E, 32)]" in _err(), (e, topk)
    assert "moe_route_fused:" in _err()


def test_grouped_entry_checks():
    for e, ng, tg, topk in ((64, 1, 1, 0), (64, 1, 1, 33), (8, 1, 1, 9), (8, 4, 2, 5)):   # 0, 33, E + 1, and one past topk_group * E / n_group
        assert _grp(e=e, ng=ng, tg=tg, topk=topk) == INVALID and "topk must be in [1, min(32, topk_group * E / n_group)]" in _err(), (e, ng, tg, topk)
    assert _grp(e=8, ng=3) == INVALID and "n_group must divide E" in _err()
    for ng in (0, 65):
        assert _grp(e=128, ng=ng) == INVALID and "n_group must be in [1, 64]" in _err()
    for tg in (0, 3):
        assert _grp(tg=tg) == INVALID and "topk_group must be in [1, n_group]" in _err()
    assert _grp(scoring=2) == INVALID and "scoring" in _err()
    assert _grp(bias=X + 2) == INVALID and "aligned" in _err()
    assert "moe_route_grouped_fused:" in _err()


# ---- the launch is a pure function --------------------------------------------------------------------------------------------------
def test_launch_plan_is_the_routers_choice_in_one_workgroup():
    lib = _lib.load()
    f = lib.qutlass_amd_debug_moe_launch_plan
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]

    def plan(op, eb, e, t, aligned, cus=256):
        out = (ctypes.c_int * 4)(-7, -7, -7, -7)
        rc = f(op, eb, e, t | (1 << 62 if aligned else 0), cus, out, 4)
        return tuple(out) if rc == 4 else None

    for eb in (2, 4):
        for e in (8, 60, 129, 1024):
            for aligned in (False, True):
                for t in (1, 9, 64):
                    one, router = plan(5, eb, e, t, aligned), plan(1, eb, e, t, aligned)
                    assert one is not None and router is not None, (eb, e, aligned, t)
                    assert one[:2] == router[:2] and one[2:] == (1, 512), (eb, e, aligned, t, one, router)
                    assert one == plan(5, eb, e, t, aligned, cus=1)                       # the CU count plays no part
                    assert one[1] == int(aligned and (e * eb) % 16 == 0)
    assert plan(5, 2, 8, 65, True) is None and plan(5, 3, 8, 4, True) is None and plan(5, 2, 1025, 4, True) is None
    assert plan(5, 2, 129, 4, True)[0] == 8 and plan(5, 4, 129, 4, True)[0] == 4 and plan(5, 2, 1024, 4, True)[0] == 16


# ---- shapes under fake tensors, tracing, schemas ------------------------------------------------------------------------------------
def _expect(res, T, topk, ne):
    assert [tuple(a.shape) for a in res] == [(T, topk), (T, topk), (T * topk,), (ne,), (T, topk)]
    assert [a.dtype for a in res] == [F32, I32, I32, I32, I32] and all(a.device.type == "cuda" for a in res)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ops_give_the_right_shapes_under_fake_tensors(dtype):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    E, topk = 64, 6
    with FakeTensorMode():
        emap = torch.empty(E, dtype=I32, device=DEV)
        bias = torch.empty(E, dtype=F32, device=DEV)
        for T in sorted({0, 1, max(_bound(), 1), _bound() + 1, 64, 65, 300}):              # below and above the bound: the same shapes
            logits = torch.empty(T, E, dtype=dtype, device=DEV)
            _expect(amd.moe_route_fused(logits, None, topk, E, True), T, topk, E)
            _expect(amd.moe_route_fused(logits, emap, topk, 8, False), T, topk, 8)
            _expect(amd.moe_route_grouped_fused(logits, None, None, topk, E, 8, 4, 0, True, 2.5), T, topk, E)
            _expect(amd.moe_route_grouped_fused(logits, bias, emap, topk, 8, 8, 4, 1, False, 1.0), T, topk, 8)
            _expect(q.moe_route_fused(logits, topk), T, topk, E)
            _expect(q.moe_route_fused(logits, topk, 8, renormalize=False, expert_map=emap), T, topk, 8)
            _expect(q.moe_route_grouped_fused(logits, topk, n_group=8, topk_group=4, bias=bias, routed_scaling_factor=2.5), T, topk, E)
            _expect(q.moe_route_grouped_fused(logits, topk, 8, n_group=8, topk_group=4, scoring="softmax", expert_map=emap), T, topk, 8)
            assert [(a.shape, a.dtype) for a in q.moe_route_fused(logits, topk)] == [(a.shape, a.dtype) for a in q.moe_route(logits, topk)]


def test_make_fx_shows_one_node():
    from torch.fx.experimental.proxy_tensor import make_fx

    q.ops.register_torch_ops()

    def caller(logits, emap):
        w, ids, src_row, offs, pos = q.moe_route_fused(logits, 2, 4, expert_map=emap)
        return w * 2.0, src_row + 1, offs, pos, ids

    with FakeTensorMode():
        gm = make_fx(caller)(torch.empty(5, 8, dtype=torch.bfloat16, device=DEV), torch.empty(8, dtype=I32, device=DEV))
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert sum("qutlass_amd.moe_route_fused" in t for t in targets) == 1, targets
    assert not any("moe_topk" in t or "moeSort" in t or "moe_sort" in t for t in targets), targets

    def grouped(logits):
        return q.moe_route_grouped_fused(logits, 2, n_group=2, topk_group=1)

    with FakeTensorMode():
        gm = make_fx(grouped)(torch.empty(5, 8, dtype=torch.bfloat16, device=DEV))
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert sum("qutlass_amd.moe_route_grouped_fused" in t for t in targets) == 1, targets


def test_a_layer_that_starts_at_moe_route_fused_traces_with_fullgraph():
    with FakeTensorMode():
        logits, emap = torch.empty(7, 16, dtype=torch.bfloat16, device=DEV), torch.empty(16, dtype=I32, device=DEV)
        r = torch.compile(lambda lg, m: q.moe_route_fused(lg, 4, 2, renormalize=False, expert_map=m), backend="eager", fullgraph=True)(logits, emap)
        _expect(r, 7, 4, 2)
        r = torch.compile(lambda lg: q.moe_route_grouped_fused(lg, 4, n_group=4, topk_group=2), backend="eager", fullgraph=True)(logits)
        _expect(r, 7, 4, 16)


def test_schemas_are_functional():
    q.ops.register_torch_ops()
    for n in ("moe_route_fused", "moe_route_grouped_fused"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments), str(schema)
        assert len(schema.returns) == 5 and not any(r.alias_info is not None for r in schema.returns), str(schema)
        assert not schema.is_mutable
        assert n not in q.ops.OUTPUT_OPS and not hasattr(torch.ops.qutlass_amd, n + "_")          # no table row, no in-place twin
    assert str(torch.ops.qutlass_amd.moe_route_fused.default._schema) == (
        "qutlass_amd::moe_route_fused(Tensor logits, Tensor? expert_map, int topk, int num_experts, bool renormalize) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")


def test_wrappers_raise_value_error():
    logits = torch.zeros(4, 8)
    for call in (lambda: q.moe_route_fused(logits, 9), lambda: q.moe_route_fused(logits, 0), lambda: q.moe_route_fused(torch.zeros(4, 64), 33),
                 lambda: q.moe_route_grouped_fused(logits, 5, n_group=4, topk_group=2)):
        with pytest.raises(ValueError, match="topk must be in"):
            call()
    for call in (lambda: q.moe_route_fused(torch.zeros(8), 2), lambda: q.moe_route_grouped_fused(torch.zeros(2, 4, 8), 2)):
        with pytest.raises(ValueError, match="logits must be"):
            call()
    empty = torch.zeros(0, dtype=I32)
    for call in (lambda: q.moe_route_fused(logits, 2, expert_map=empty), lambda: q.moe_route_grouped_fused(logits, 2, expert_map=empty)):
        with pytest.raises(ValueError, match="expert_map must have"):
            call()
    with pytest.raises(ValueError, match="n_group must divide E"):
        q.moe_route_grouped_fused(logits, 2, n_group=3)
    with pytest.raises(ValueError, match="scoring must be"):
        q.moe_route_grouped_fused(logits, 2, scoring="tanh")
    with pytest.raises(ValueError, match="bias must be"):
        q.moe_route_grouped_fused(logits, 2, bias=torch.zeros(7))


def test_alias_package_exposes_the_new_functions():
    import qutlass

    for n in ("moe_route_fused", "moe_route_grouped_fused"):
        assert getattr(qutlass, n) is getattr(q, n)
