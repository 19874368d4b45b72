"""moe_combine with the down projection's per-expert bias on the GPU: byte for byte moe_combine(y + bias[g(rows)], pos, weights) with torch's bf16 add, the numpy
model (tests/_swiglu_oai_model.py), dropped slots next to NaNs, and the unchanged op without a bias.  The CPU half is tests/test_swiglu_oai_cpu.py."""
import numpy as np
import pytest
import torch

import _swiglu_oai_model as model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _np(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.numpy()


def _offs_patterns(M):
    """(name, E, counts): tests/test_gpu_moe_grouped_scales.py's patterns -- boundaries at rows 31 / 32 / 33, empty groups, E = 65 and 1024, a tail past offs[E - 1]"""
    def counts(E, owners, total):
        c = np.zeros(E, dtype=np.int64)
        for i in range(total):
            c[owners[i % len(owners)]] += 1
        return c

    e3 = np.diff([0, min(31, M), min(32, M), min(33, M)])
    e5 = np.array([M - 1 - (M - 1) // 3, 0, 1, 0, (M - 1) // 3])
    return [("E1", 1, np.array([M])), ("E3", 3, e3), ("E5", 5, e5), ("E65", 65, counts(65, list(range(64, -1, -1)) if M < 65 else list(range(65)), M)),
            ("E1024", 1024, counts(1024, [517, 3, 1023], M)), ("E5tail", 5, counts(5, [0, 2, 3], M - min(7, M - 1)))]


def _experts(offs, M):
    return torch.searchsorted(offs.to(torch.int64), torch.arange(M, device=DEV), right=True).clamp(max=offs.numel() - 1)


def _case(T, topk, H, gen, drop=True):
    """y (M, H), pos (T, topk) a permutation of the M = T * topk rows with a few slots dropped (-1 or >= M), weights"""
    M = T * topk
    y = (torch.randn(M, H, generator=gen) * 2.0).to(torch.bfloat16)
    pos = torch.randperm(M, generator=gen).to(torch.int32).view(T, topk)
    if drop and M > 2:
        flat = pos.view(-1)
        flat[1] = -1
        flat[M // 2] = M + 3
    w = torch.rand(T, topk, generator=gen) + 0.1
    return y.to(DEV), pos.to(DEV), w.to(DEV)


@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("topk", [1, 4, 5, 32])
def test_bias_equals_torch_add_then_combine(q, T, topk):
    gen = torch.Generator(device="cpu").manual_seed(T * 100 + topk)
    for H in (8, 136):
        y, pos, w = _case(T, topk, H, gen)
        M = y.size(0)
        for name, E, counts in _offs_patterns(M):
            bias = (torch.randn(E, H, generator=gen) * 2.0).to(torch.bfloat16)
            assert len({r.numpy().tobytes() for r in bias.view(torch.int16)}) == E          # pairwise different: a wrong expert changes bytes
            bias, offs = bias.to(DEV), torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
            got = q.moe_combine(y, pos, w, bias=bias, offs=offs)
            want = q.moe_combine(y + bias[_experts(offs, M)], pos, w)
            assert got.shape == (T, H) and got.dtype == torch.bfloat16
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (T, topk, H, name)
            live = (pos >= 0) & (pos < M)
            if bool((_experts(offs, M)[pos[live].long()] > 0).any()):   # the precondition: where a live slot names another expert's row, expert 0's bias gives other bytes
                assert not torch.equal(q.moe_combine(y + bias[0], pos, w).view(torch.int16), want.view(torch.int16)), (T, topk, H, name)
            if E == 1:
                assert torch.equal(q.moe_combine(y, pos, w, bias=bias).view(torch.int16), want.view(torch.int16))
    torch.cuda.synchronize()


def test_bit_equal_to_the_numpy_model(q):
    gen = torch.Generator(device="cpu").manual_seed(3)
    y, pos, w = _case(33, 5, 136, gen)
    counts = np.array([40, 0, 50, 1, 60])                                   # 151 of 165 rows: a tail under expert 4
    bias = (torch.randn(5, 136, generator=gen) * 2.0).to(torch.bfloat16).to(DEV)
    offs = torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
    got = q.moe_combine(y, pos, w, bias=bias, offs=offs)
    want = model.moe_combine_bias(_np(y), _np(pos), _np(w), _np(bias), np.cumsum(counts))
    assert np.array_equal(_np(got), want), int((_np(got) != want).sum())


def test_dropped_slots_and_unreferenced_nans(q):
    gen = torch.Generator(device="cpu").manual_seed(4)
    T, topk, H, E = 9, 4, 136, 4
    M = 40
    y = (torch.randn(M, H, generator=gen) * 2.0).to(torch.bfloat16)
    bias = (torch.randn(E, H, generator=gen) * 2.0).to(torch.bfloat16)
    offs = torch.tensor([10, 20, 30, 40], dtype=torch.int32)
    pos = torch.randint(0, 10, (T, topk), generator=gen, dtype=torch.int32)   # every referenced row belongs to expert 0 ...
    pos[:, 1] = torch.randint(20, 30, (T,), generator=gen, dtype=torch.int32)  # ... or expert 2
    pos[0, :] = torch.tensor([-1, M, -7, 2 ** 31 - 1], dtype=torch.int32)      # a token whose slots are all dropped
    pos[1, 0], pos[2, 3] = -1, M + 5
    ref = torch.zeros(M, dtype=torch.bool)
    ok = (pos >= 0) & (pos < M)
    ref[pos[ok].long()] = True
    y[~ref] = float("nan")                                                     # unreferenced rows of y (row 0, which skipped slots load, may be among them)
    bias[1] = float("nan")                                                     # experts that own no referenced row
    bias[3] = float("nan")
    w = torch.rand(T, topk, generator=gen) + 0.1
    y, pos, w, bias, offs = (t.to(DEV) for t in (y, pos, w, bias, offs))
    got = q.moe_combine(y, pos, w, bias=bias, offs=offs)
    assert bool(torch.isfinite(got.float()).all())
    assert (_np(got[0]) == 0).all()                                            # all slots dropped: +0, bit for bit
    want = model.moe_combine_bias(_np(y), _np(pos), _np(w), _np(bias), _np(offs))
    assert np.array_equal(_np(got), want)


def test_without_a_bias_it_is_todays_op(q):
    gen = torch.Generator(device="cpu").manual_seed(5)
    y, pos, w = _case(33, 4, 136, gen)
    a = q.moe_combine(y, pos, w, bias=None, offs=None)
    out = torch.empty_like(a)
    torch.ops.qutlass_amd.moeCombine_(y, pos, w, out)
    assert torch.equal(a.view(torch.int16), out.view(torch.int16))
    zero = torch.zeros(1, 136, dtype=torch.bfloat16, device=DEV)               # a zero bias adds +0: the same bytes unless y holds -0 (it does not here)
    assert torch.equal(q.moe_combine(y, pos, w, bias=zero).view(torch.int16), a.view(torch.int16))
