"""MoE dispatch and combine (moe_sort, fusedGatherQuantize{Mx,Nv}, moe_combine) without a GPU: the C ABI's argument checks (every one of them happens before any HIP
call, so null / dummy pointers are enough), moe_sort on CPU tensors against numpy, the shape-only kernels of the torch ops, tracing of a whole MoE layer, and the Python
wrappers' own errors.  The GPU half is tests/test_gpu_moe_dispatch.py."""
import ctypes

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib

DEV = "cuda"
OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def test_the_three_symbols_are_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qutlass_amd_fused_gather_quantize_mx", "qutlass_amd_fused_gather_quantize_nv", "qutlass_amd_moe_combine_bf16"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def _mx(rot, t, k, m, method=0, x=X, h=X, src=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_gather_quantize_mx(x, h, rot, t, k, src, m, method, out, sf, None)


def _nv(rot, t, k, m, method=1, x=X, h=X, src=X, gs=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_gather_quantize_nv(x, h, rot, t, k, src, m, method, gs, out, sf, None)


def test_gather_quantize_argument_checks():
    for call, rots, bad_rots in ((_mx, (32, 64, 128), (16, 0, 48, 256)), (_nv, (16, 32, 64, 128), (8, 0, 48, 256))):
        for rot in rots:
            rp = max(rot, 32)
            assert call(rot, 4, rp, 0) == OK                                              # M == 0 returns before any launch
            assert call(rot, 4, rp, 0, x=None, h=None, src=None, out=None, sf=None) == OK
            assert call(rot, 4, rp + 16, 4) == INVALID and f"multiple of {rp}" in _err()   # K % max(rot, 32)
            assert call(rot, 4, 0, 4) == INVALID and "bad shape" in _err()
            assert call(rot, -1, rp, 4) == INVALID and "bad shape" in _err()
            assert call(rot, 4, rp, -1) == INVALID and "bad shape" in _err()
            assert call(rot, 4, -rp, 4) == INVALID and "bad shape" in _err()
            assert call(rot, 1 << 31, rp, 4) == INVALID and "bad shape" in _err()
            for method in (-1, 2):
                assert call(rot, 4, rp, 4, method=method) == INVALID and "invalid method" in _err()
            assert call(rot, 4, rp, 4, x=X + 4) == INVALID and "16-byte aligned" in _err()
            for null in ("x", "h", "src", "out", "sf"):
                assert call(rot, 4, rp, 4, **{null: None}) == INVALID and "null pointer" in _err(), null
        for rot in bad_rots:
            assert call(rot, 4, 256, 4) == INVALID and "Unsupported rotation size" in _err()
    assert _nv(32, 4, 64, 4, gs=None) == INVALID and "null pointer" in _err()
    assert _mx(64, 4, 64, 4, h=X + 2) == INVALID and "rotation matrix must be 16-byte aligned" in _err()


def test_gather_quantize_size_limit_is_checked_not_wrapped():
    """x = T * K * 2 bytes must stay below 2 GiB (32-bit offsets from one buffer descriptor, and offset 2^31 is the kernel's zero row): the first size beyond it is
    refused, for both formats and however the 2^30 elements split into rows and columns; M == 0 with a legal x still returns OK."""
    t, k = 1 << 15, 1 << 15        # T * K = 2^30: exactly 2 GiB of input
    assert _mx(32, t, k, 4) == INVALID and "below 2 GiB" in _err()
    assert _nv(16, t, k, 4) == INVALID and "below 2 GiB" in _err()
    assert _mx(128, (1 << 30) // 128, 128, 4) == INVALID and "below 2 GiB" in _err()
    assert _mx(32, t, k, 0) == INVALID and "below 2 GiB" in _err()           # (the size checks come before the M == 0 return)
    assert _mx(32, t - 1, k, 0) == OK and _nv(16, t, k - 32, 0) == OK        # the last sizes below it pass the check


def _cb(m, hd, t, topk, y=X, pos=X, w=X, out=X):
    return _lib.load().qutlass_amd_moe_combine_bf16(y, m, hd, pos, w, t, topk, out, None)


def test_moe_combine_argument_checks():
    assert _cb(4, 64, 0, 2) == OK                                      # T == 0: nothing to do
    assert _cb(4, 64, 0, 2, y=None, pos=None, w=None, out=None) == OK
    assert _cb(4, 12, 3, 2) == INVALID and "multiple of 8" in _err()
    assert _cb(4, 0, 3, 2) == INVALID and "bad shape" in _err()
    assert _cb(-1, 64, 3, 2) == INVALID and "bad shape" in _err()
    assert _cb(4, 64, -1, 2) == INVALID and "bad shape" in _err()
    assert _cb(1 << 31, 64, 3, 2) == INVALID and "bad shape" in _err()
    assert _cb(4, 64, 1 << 31, 2) == INVALID and "bad shape" in _err()
    for topk in (0, -1, 33):
        assert _cb(4, 64, 3, topk) == INVALID and "bad shape" in _err()
    assert _cb(4, 64, 3, 2, y=X + 2) == INVALID and "16-byte aligned" in _err()
    assert _cb(4, 64, 3, 2, out=X + 8) == INVALID and "16-byte aligned" in _err()
    for null in ("y", "pos", "w", "out"):
        assert _cb(4, 64, 3, 2, **{null: None}) == INVALID and "null pointer" in _err(), null


# ---- moe_sort on CPU tensors ------------------------------------------------------------------------------------------------------
def _check_sort(ids: np.ndarray, E: int, dtype=torch.int64):
    T, topk = ids.shape
    src_row, offs, pos = q.moe_sort(torch.from_numpy(ids).to(dtype), E)
    assert src_row.shape == (T * topk,) and offs.shape == (E,) and pos.shape == (T, topk)
    assert src_row.dtype == offs.dtype == pos.dtype == torch.int32
    src_row, offs, pos = src_row.numpy(), offs.numpy(), pos.numpy()
    flat = ids.reshape(-1)
    kept = (flat >= 0) & (flat < E)
    key = np.where(kept, flat, E)
    order = np.argsort(key, kind="stable")
    assert np.array_equal(src_row, order // topk)                                      # the numpy stable argsort
    assert np.array_equal(offs, np.cumsum(np.bincount(flat[kept], minlength=E)))       # cumulative histogram of the kept ids
    want_pos = np.empty(T * topk, dtype=np.int64)
    want_pos[order] = np.arange(T * topk)
    assert np.array_equal(pos.reshape(-1), np.where(kept, want_pos, -1))
    p = pos.reshape(-1)
    assert (p[~kept] == -1).all() and (p[kept] < offs[-1]).all()                       # dropped slots: -1, and they do not count in offs
    assert np.array_equal(src_row[p[kept]], np.nonzero(kept)[0] // topk)               # src_row[pos[t, k]] == t for every kept slot
    assert len(set(p[kept].tolist())) == int(kept.sum())
    # every expert's rows are its own, in (token, slot) order
    start = 0
    for e in range(E):
        rows = np.nonzero(flat == e)[0]
        assert np.array_equal(order[start:offs[e]], rows), e
        start = offs[e]


def test_moe_sort_matches_a_numpy_stable_argsort():
    rng = np.random.default_rng(0)
    _check_sort(np.array([[2, 0]]), 4)                                                 # T = 1
    _check_sort(np.array([[3]]), 4)
    _check_sort(rng.integers(0, 4, (35, 2)) * 2 % 5 % 4, 4)
    ids = rng.integers(0, 4, (35, 2))
    ids[ids == 1] = 3                                                                  # an empty expert
    _check_sort(ids, 4)
    _check_sort(np.full((9, 3), 2), 4)                                                 # all tokens in one expert
    ids = rng.integers(0, 6, (33, 4))
    ids[::3, 1] = -1                                                                   # dropped ids: -1 and E
    ids[1::5, 2] = 6
    _check_sort(ids, 6)
    _check_sort(ids.astype(np.int32), 6, torch.int32)
    _check_sort(np.full((4, 2), -1), 3)                                                # everything dropped: offs all zero
    _check_sort(np.zeros((0, 2), dtype=np.int64), 3)                                   # no tokens
    with pytest.raises(ValueError, match="topk_ids must be"):
        q.moe_sort(torch.zeros(4, dtype=torch.int64), 3)


# ---- shapes under fake tensors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [70, 140])
def test_ops_give_the_plain_quantizers_shapes_under_fake_tensors(m):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    t, k = 33, 384
    with FakeTensorMode():
        x = torch.empty(t, k, dtype=torch.bfloat16, device=DEV)
        src = torch.empty(m, dtype=torch.int32, device=DEV)
        plain = torch.empty(m, k, dtype=torch.bfloat16, device=DEV)
        h = torch.empty(32, 32, dtype=torch.bfloat16, device=DEV)
        gs = torch.empty(1, device=DEV)
        c, s = amd.gather_quantize_mx(x, h, src, 0)
        pc, ps = amd.quantize_mx(plain, h, 0)
        assert c.shape == pc.shape == (m, k // 2) and c.dtype == pc.dtype == torch.uint8 and c.device.type == "cuda"
        assert s.shape == ps.shape == ((m + 127) // 128 * 128, 12) and s.dtype == ps.dtype == torch.float8_e8m0fnu
        c, s = amd.gather_quantize_nv(x, h, src, gs, 1)
        pc, ps = amd.quantize_nv(plain, h, gs, 1)
        assert c.shape == pc.shape == (m, k // 2) and c.dtype == torch.uint8
        assert s.shape == ps.shape == ((m + 127) // 128 * 128, 24) and s.dtype == ps.dtype == torch.float8_e4m3fn
        # the eager wrappers (in-place twins on tensors they allocate) agree with the plain quantizers on an (M, K) tensor
        for got, want in ((q.fusedGatherQuantizeMx(x, h, src), q.fusedQuantizeMx(plain, h)),
                          (q.fusedGatherQuantizeMx(x, h, src, method="abs_max"), q.fusedQuantizeMx(plain, h, method="abs_max")),
                          (q.fusedGatherQuantizeNv(x, h, gs, src), q.fusedQuantizeNv(plain, h, gs)),
                          (q.fusedGatherQuantizeNv(x, h, gs, src, method="quest"), q.fusedQuantizeNv(plain, h, gs, method="quest"))):
            assert [(a.shape, a.dtype, a.device.type) for a in got] == [(a.shape, a.dtype, a.device.type) for a in want]
        y = torch.empty(m, 256, dtype=torch.bfloat16, device=DEV)
        pos = torch.empty(t, 2, dtype=torch.int32, device=DEV)
        w = torch.empty(t, 2, device=DEV)
        for out in (amd.moe_combine(y, pos, w), q.moe_combine(y, pos, w)):
            assert out.shape == (t, 256) and out.dtype == torch.bfloat16 and out.device.type == "cuda"


def test_in_place_twins_declare_their_writes():
    q.ops.register_torch_ops()
    q.ops.register_torch_ops()   # (idempotent)
    for n, nwritten in (("fusedGatherQuantizeMx_", 2), ("fusedGatherQuantizeNv_", 2), ("moeCombine_", 1)):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert len(written) == nwritten and len(schema.returns) == 0, str(schema)
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{n}").fake_impl.kernel is not None
    for n in ("gather_quantize_mx", "gather_quantize_nv", "moe_combine"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments), str(schema)


def test_a_whole_moe_layer_traces_with_fullgraph():
    E, H, I, T, topk = 4, 256, 128, 35, 2

    def layer(x, topk_ids, topk_w, h, w13q, w13s, w2q, w2s, alpha):
        src_row, offs, pos = q.moe_sort(topk_ids, E)
        aq, asf = q.fusedGatherQuantizeMx(x, h, src_row, method="abs_max")
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        y = q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs)
        return q.moe_combine(y, pos, topk_w)

    with FakeTensorMode():
        args = (torch.empty(T, H, dtype=torch.bfloat16, device=DEV), torch.empty(T, topk, dtype=torch.int64, device=DEV), torch.empty(T, topk, device=DEV),
                torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(E, 2 * I, H // 2, dtype=torch.uint8, device=DEV), torch.empty(E * 2 * I * H // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(E, H, I // 2, dtype=torch.uint8, device=DEV), torch.empty(E * H * I // 32, dtype=torch.float8_e8m0fnu, device=DEV),
                torch.empty(1, device=DEV))
        out = torch.compile(layer, backend="eager", fullgraph=True)(*args)
        assert out.shape == (T, H) and out.dtype == torch.bfloat16
        s, o, p = torch.compile(lambda ids: q.moe_sort(ids, E), backend="eager", fullgraph=True)(args[1])
        assert s.shape == (T * topk,) and o.shape == (E,) and p.shape == (T, topk) and s.dtype == o.dtype == p.dtype == torch.int32


def test_bad_method_raises_value_error():
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    h = torch.zeros(32, 32, dtype=torch.bfloat16)
    src = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: q.fusedGatherQuantizeMx(x, h, src, method="nope"), lambda: q.fusedGatherQuantizeNv(x, h, torch.ones(1), src, method="nope")):
        with pytest.raises(ValueError, match="invalid method 'nope', must be 'quest' or 'abs_max'"):
            call()


def test_alias_package_exposes_the_new_functions():
    import qutlass

    for n in ("moe_sort", "fusedGatherQuantizeMx", "fusedGatherQuantizeNv", "moe_combine"):
        assert getattr(qutlass, n) is getattr(q, n)
