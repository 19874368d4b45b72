"""MoE routing (moe_topk_softmax, moe_sort_fused, moe_route) without a GPU: the exported symbols and the header, the C ABI's argument checks (every one of them
happens before any HIP call, so null / dummy pointers are enough), the workspace query, the shape-only kernels of the torch ops, tracing of a layer that starts at
the router's logits, and the Python wrappers' own errors.  The GPU half is tests/test_gpu_moe_route.py."""
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
NAMES = ("qutlass_amd_moe_topk_softmax", "qutlass_amd_moe_sort", "qutlass_amd_moe_sort_workspace_bytes")


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def test_the_three_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
        assert f"{name}(" in header, name


def _tk(t, e, topk, eb=2, renorm=1, logits=X, w=X, ids=X):
    return _lib.load().qutlass_amd_moe_topk_softmax(logits, eb, t, e, topk, renorm, w, ids, None)


def test_topk_softmax_argument_checks():
    assert _tk(0, 8, 2) == OK                                                  # T == 0: nothing to do
    assert _tk(0, 8, 2, logits=None, w=None, ids=None) == OK
    for eb in (0, 1, 3, 8):
        assert _tk(4, 8, 2, eb=eb) == INVALID and "elem_bytes" in _err()
    assert _tk(-1, 8, 2) == INVALID and "bad shape" in _err()
    assert _tk(1 << 31, 8, 2) == INVALID and "bad shape" in _err()
    for e in (0, -1, 1025):
        assert _tk(4, e, 1) == INVALID and "number of experts" in _err()
    for e, topk in ((8, 0), (8, -1), (8, 9), (1, 2), (64, 33), (1024, 33)):
        assert _tk(4, e, topk) == INVALID and "topk must be in [1, min(E, 32)]" in _err(), (e, topk)
    assert _tk(4, 8, 2, logits=X + 1) == INVALID and "aligned" in _err()
    assert _tk(4, 8, 2, eb=4, logits=X + 2) == INVALID and "aligned" in _err()
    assert _tk(4, 8, 2, w=X + 2) == INVALID and "aligned" in _err()
    assert _tk(4, 8, 2, ids=X + 1) == INVALID and "aligned" in _err()
    for null in ("logits", "w", "ids"):
        assert _tk(4, 8, 2, **{null: None}) == INVALID and "null pointer" in _err(), null


def _st(t, topk, e, ib=4, ids=X, emap=None, g=0, src=X, offs=X, pos=X, ws=None, wsb=0):
    return _lib.load().qutlass_amd_moe_sort(ids, ib, t, topk, e, emap, g, src, offs, pos, ws, wsb, None)


def _ws(n, e):
    return _lib.load().qutlass_amd_moe_sort_workspace_bytes(n, e)


def _bound(e):
    lo, hi = 1, 1 << 30
    assert _ws(lo, e) == 0 and _ws(hi, e) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _ws(mid, e) == 0 else (lo, mid)
    return lo


def test_sort_argument_checks():
    assert _st(0, 2, 8) == OK                                                  # no slots: nothing to do
    assert _st(0, 2, 8, ids=None, src=None, offs=None, pos=None) == OK
    for ib in (0, 2, 16):
        assert _st(4, 2, 8, ib=ib) == INVALID and "id_bytes" in _err()
    assert _st(-1, 2, 8) == INVALID and "bad shape" in _err()
    assert _st(4, 0, 8) == INVALID and "bad shape" in _err()
    assert _st(4, -2, 8) == INVALID and "bad shape" in _err()
    assert _st(1 << 28, 8, 8) == INVALID and "T * topk < 2^31" in _err()       # exactly 2^31 slots
    assert _st(1 << 31, 1, 8) == INVALID and "bad shape" in _err()
    for e in (0, -3, 1025):
        assert _st(4, 2, e) == INVALID and "number of experts" in _err()
    assert _st(4, 2, 8, emap=X, g=-1) == INVALID and "expert_map" in _err()
    assert _st(4, 2, 8, emap=X, g=1 << 31) == INVALID and "expert_map" in _err()
    assert _st(4, 2, 8, ib=8, ids=X + 4) == INVALID and "aligned" in _err()
    for arg in ("ids", "emap", "src", "offs", "pos", "ws"):
        assert _st(4, 2, 8, **{arg: X + 2}, **({"g": 4} if arg == "emap" else {})) == INVALID and "aligned" in _err(), arg
    for null in ("ids", "src", "offs", "pos"):
        assert _st(4, 2, 8, **{null: None}) == INVALID and "null pointer" in _err(), null
    # beyond the one-launch bound the scratch is required, whole
    n = _bound(8) + 1
    need = _ws(n, 8)
    assert need > 0
    assert _st(n, 1, 8) == INVALID and "workspace" in _err()
    assert _st(n, 1, 8, ws=X, wsb=need - 1) == INVALID and "workspace" in _err()
    assert _st(n, 1, 8, ws=None, wsb=need) == INVALID and "workspace" in _err()


def test_workspace_bytes_is_zero_up_to_the_bound_and_monotone_beyond():
    for e in (1, 8, 128, 1024):
        b = _bound(e)
        assert b >= 4096 and b == _bound(1)                                    # at least 4096 slots in one launch; the bound does not depend on E
        assert all(_ws(n, e) == 0 for n in (0, 1, 64, 4096, b))
        prev = 0
        for n in [b + 1, b + 2, 2 * b, 40000, 131072, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 28, (1 << 31) - 1]:
            if n <= b:
                continue
            cur = _ws(n, e)
            assert cur >= prev > -1 and cur > 0 and cur % 4 == 0 and cur <= 257 * (e + 1) * 4, (n, e, cur)
            prev = cur
        assert _ws(b + 1, e) >= 2 * (e + 1) * 4
    assert _ws(40000, 1024) > _ws(40000, 8)
    assert _ws(-5, 8) == 0 and _ws(1 << 31, 8) == 0 and _ws(40000, 0) == 0 and _ws(40000, 1025) == 0   # nothing to size for a shape the sort refuses


# ---- shapes under fake tensors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ops_give_the_right_shapes_under_fake_tensors(dtype):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    T, E, topk = 33, 60, 6
    with FakeTensorMode():
        logits = torch.empty(T, E, dtype=dtype, device=DEV)
        for w, ids in (amd.moe_topk_softmax(logits, topk, True), q.moe_topk_softmax(logits, topk), q.moe_topk_softmax(logits, topk, renormalize=False)):
            assert w.shape == ids.shape == (T, topk) and w.dtype == torch.float32 and ids.dtype == torch.int32 and w.device.type == ids.device.type == "cuda"
        emap = torch.empty(E, dtype=torch.int32, device=DEV)
        for idt in (torch.int32, torch.int64):
            tids = torch.empty(T, topk, dtype=idt, device=DEV)
            for res in (amd.moe_sort_fused(tids, None, E), amd.moe_sort_fused(tids, emap, 8), q.moe_sort_fused(tids, E), q.moe_sort_fused(tids, 8, expert_map=emap)):
                s, o, p = res
                assert s.shape == (T * topk,) and p.shape == (T, topk) and o.shape[0] in (E, 8)
                assert s.dtype == o.dtype == p.dtype == torch.int32 and s.device.type == "cuda"
            want = q.moe_sort(tids, E)
            assert [(a.shape, a.dtype) for a in q.moe_sort_fused(tids, E)] == [(a.shape, a.dtype) for a in want]
        big = torch.empty(_bound(E) // 8 + 1, 8, dtype=torch.int32, device=DEV)   # the three-launch form: the wrapper sizes the scratch without a device
        assert q.moe_sort_fused(big, E)[0].shape == (big.numel(),)
        r = q.moe_route(logits, topk)
        assert [tuple(a.shape) for a in r] == [(T, topk), (T, topk), (T * topk,), (E,), (T, topk)]
        assert q.moe_route(logits, topk, 8, expert_map=emap)[3].shape == (8,)
        assert q.moe_topk_softmax(torch.empty(0, E, dtype=dtype, device=DEV), topk)[0].shape == (0, topk)


def test_in_place_twins_declare_their_writes():
    q.ops.register_torch_ops()
    for n, nwritten in (("moeTopkSoftmax_", 2), ("moeSort_", 4)):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert len(written) == nwritten and len(schema.returns) == 0, str(schema)
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{n}").fake_impl.kernel is not None
    for n in ("moe_topk_softmax", "moe_sort_fused"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments), str(schema)


def test_a_layer_that_starts_at_moe_route_traces_with_fullgraph():
    E, H, I, T, topk = 4, 256, 128, 35, 2

    def layer(x, logits, h, w13q, w13s, w2q, w2s, alpha):
        topk_w, _, src_row, offs, pos = q.moe_route(logits, topk)
        aq, asf = q.fusedGatherQuantizeMx(x, h, src_row, method="abs_max")
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        y = q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs)
        return q.moe_combine(y, pos, topk_w)

    with FakeTensorMode():
        args = (torch.empty(T, H, dtype=torch.bfloat16, device=DEV), torch.empty(T, E, dtype=torch.bfloat16, device=DEV),
                torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(E, 2 * I, H // 2, dtype=torch.uint8, device=DEV), torch.empty(E * 2 * I * H // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(E, H, I // 2, dtype=torch.uint8, device=DEV), torch.empty(E * H * I // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(1, device=DEV))
        out = torch.compile(layer, backend="eager", fullgraph=True)(*args)
        assert out.shape == (T, H) and out.dtype == torch.bfloat16
        emap = torch.empty(16, dtype=torch.int32, device=DEV)
        r = torch.compile(lambda lg, m: q.moe_route(lg, topk, 2, renormalize=False, expert_map=m), backend="eager", fullgraph=True)(args[1], emap)
        assert [tuple(a.shape) for a in r] == [(T, topk), (T, topk), (T * topk,), (2,), (T, topk)]


def test_wrappers_raise_value_error():
    logits = torch.zeros(4, 8)
    for call in (lambda: q.moe_topk_softmax(logits, 9), lambda: q.moe_topk_softmax(logits, 0), lambda: q.moe_route(logits, 9),
                 lambda: q.moe_topk_softmax(torch.zeros(4, 64), 33)):
        with pytest.raises(ValueError, match="topk must be in"):
            call()
    for call in (lambda: q.moe_topk_softmax(torch.zeros(8), 2), lambda: q.moe_route(torch.zeros(2, 4, 8), 2)):
        with pytest.raises(ValueError, match="logits must be"):
            call()
    with pytest.raises(ValueError, match="topk_ids must be"):
        q.moe_sort_fused(torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="expert_map must have"):   # an empty tensor is the in-place op's "no map"
        q.moe_sort_fused(torch.zeros(4, 2, dtype=torch.int32), 3, expert_map=torch.zeros(0, dtype=torch.int32))


def test_alias_package_exposes_the_new_functions():
    import qutlass

    for n in ("moe_topk_softmax", "moe_sort_fused", "moe_route"):
        assert getattr(qutlass, n) is getattr(q, n)
