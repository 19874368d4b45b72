"""grouped_matmul_bf16_nvf4_bf16_tn on the MI355X against fp64 dequantise + matmul + one rounding to bf16 (tests/_bf16_nvf4_model.py).  The plan entry tells which
form (620, 621) the product runs; the exact cases also force each form through the lab library.  Their operands are asserted exact in tests/test_grouped_bf16_nvf4_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _bf16_nvf4_model as W  # noqa: E402
import qutlass_amd as q  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0x7B7B   # bf16 bits no case produces
ARBITRARY = [([40, 30], 620), ([1030], 621)]   # (counts, the form the rule picks) at N = 40, K = 384


_offs = lambda counts: torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
_bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
_want_bits = lambda ref64: W.to_bf16_bits(ref64).numpy().view(np.uint16)
_plan = lambda M, N, K, E: q._lib.load().qutlass_amd_debug_grouped_bf16_nvf4_plan(*map(ctypes.c_int64, (M, N, K, E)), None)


def _runs(ops, shape, offs, alpha, src_row=None):
    """{name: bits} of the C entry into a sentinel-filled D: the product library under its rule, the lab library with each form forced"""
    (x, b, bsf), (M, N, K, E), name, out = ops, shape, "qutlass_amd_grouped_matmul_bf16_nvf4_bf16_tn", {}
    for who, lib, v in (("product", q._lib.load(), 0), (620, lab.load(), 620), (621, lab.load(), 621)):
        D = torch.full((M, N), SENTINEL, dtype=torch.int16, device=DEV)
        f = getattr(lib, name)
        f.restype, f.argtypes = q._lib.SYMBOLS[name]
        with lab.forced(gemm_variant=v):
            rc = f(x.data_ptr(), b.data_ptr(), bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), src_row.data_ptr() if src_row is not None else None,
                   x.size(0) if src_row is not None else 0, D.data_ptr(), M, N, K, E, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.qutlass_amd_last_error().decode()
        out[who] = _bits(D)
    return out


@pytest.mark.parametrize("E,nan", [(1, ()), (8, ()), (2, ((1, 5, 11, 0x7F), (1, 20, 12, 0xFF)))])
def test_every_scale_byte_times_every_code(E, nan):
    """one-hot tokens read the dequantised weight out: out[j, n] == w[g(j), n, j], bit-equal where non-zero -- 256 rows in one group and split into 8 groups of 32
    (the rule picks 620 for both), each form forced; the groups read out carry all 254 finite bytes in either split.  With NaN bytes planted in two (row, group)
    places of expert 1 of 2: NaN in exactly those weight rows' columns for that expert's rows (x * NaN is NaN for x = 0 too), everything else as before"""
    p = W.every_byte_problem(E)
    rows = p.M // E
    assert _plan(p.M, p.N, p.K, E) == 620
    assert nan or len(np.unique(np.concatenate([p.sfb[g][:, g * rows // 16:(g + 1) * rows // 16].ravel() for g in range(E)]))) == 254
    want_nan = np.zeros((p.M, p.N), bool)
    for g, n, grp, byte in nan:
        p.sfb[g, n, grp] = byte
        want_nan[g * rows:(g + 1) * rows, n] = True
    w = p.b_f64()                                                # (E, N, K)
    want64 = np.stack([w[j // rows, :, j] for j in range(p.M)])  # (M, N): finite wherever the row's own group is
    ref = W.reference_f64(p, [rows] * E)
    assert np.array_equal(np.isnan(ref), want_nan) and np.array_equal(ref[~want_nan], want64[~want_nan])
    want, nz = _want_bits(np.nan_to_num(ref)), ~want_nan & (ref != 0)
    for name, got in _runs(p.device(DEV), (p.M, p.N, p.K, E), _offs([rows] * E), torch.ones(1, device=DEV)).items():
        assert np.array_equal((got & 0x7FFF) > 0x7F80, want_nan), name
        assert np.array_equal(got[nz], want[nz]) and not (got[~want_nan & ~nz] & 0x7FFF).any(), name


@pytest.mark.parametrize("K,N", W.LADDER)
def test_exact_ladder_bit_equal_to_fp64(K, N):
    """every rung of the slot ladder and ragged N, the rule's form and each forced one, sorted tokens and src_row: bit for bit; rows past offs[E-1] keep the sentinel"""
    p, alpha, unsorted, src, seen = W.ladder_case(K, N)
    counts, end, (x, b, bsf) = W.COUNTS, sum(W.COUNTS), p.device(DEV)
    xu, src_d = torch.from_numpy(unsorted.view(np.int16)).to(DEV).view(torch.bfloat16), torch.from_numpy(src).to(DEV)
    al, offs = torch.tensor(alpha, dtype=torch.float32, device=DEV), _offs(counts)
    assert _plan(p.M, N, K, p.E) == 620
    for ops, sr, ref in (((x, b, bsf), None, W.reference_f64(p, counts, alpha)), ((xu, b, bsf), src_d, W.reference_f64(p, counts, alpha, x=seen))):
        want = _want_bits(ref)
        for name, got in _runs(ops, (p.M, N, K, p.E), offs, al, sr).items():
            assert np.array_equal(got[:end], want[:end]), (name, sr is not None, int((got[:end] != want[:end]).sum()))
            assert (got[end:] == SENTINEL).all(), (name, "rows past offs[E-1] were written")


@pytest.mark.parametrize("counts,want_form", ARBITRARY)
def test_arbitrary_operands_within_the_derived_bound(counts, want_form):
    """|out - ref| <= 2^-8 |ref| + K 2^-23 |alpha| sum_k |x w|: one bf16 rounding plus the worst-case fp32 accumulation error"""
    E, N, K, M = len(counts), 40, 384, sum(counts)
    rng = np.random.default_rng(M)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(torch.bfloat16)
    p = W.NvW4A16(x.view(torch.int16).numpy().view(np.uint16), rng.integers(0, 256, (E, N, K // 2)), W.FINITE[rng.integers(0, len(W.FINITE), (E, N, K // 16))])
    alpha = rng.uniform(0.5, 2.0, E).astype(np.float32)
    assert _plan(M, N, K, E) == want_form
    got = q.grouped_matmul_bf16_nvf4_bf16_tn(*p.device(DEV), torch.from_numpy(alpha).to(DEV), _offs(counts)).float().cpu().numpy().astype(np.float64)
    ref = W.reference_f64(p, counts, alpha)
    mag = W.reference_f64(W.NvW4A16(p.x & 0x7FFF, p.b & 0x77, p.sfb & 0x7F), counts, np.abs(alpha))   # alpha sum |x| |w|: every sign bit cleared
    assert (np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + K * 2.0 ** -23 * mag).all()


def test_the_cases_meet_both_forms_and_the_dense_wrapper_is_one_expert():
    assert {_plan(sum(c), 40, 384, len(c)) for c, _ in ARBITRARY} | {_plan(sum(W.COUNTS) + 5, N, K, len(W.COUNTS)) for K, N in W.LADDER} == {620, 621}
    p = W.exact_problem(1, 24, 640, 45, seed=5)
    (x, b, bsf), al = p.device(DEV), torch.full((1,), 0.5, device=DEV)
    dense = q.matmul_bf16_nvf4_bf16_tn(x, b[0], bsf, al)
    assert torch.equal(dense.view(torch.int16), q.grouped_matmul_bf16_nvf4_bf16_tn(x, b, bsf, al, _offs([45])).view(torch.int16))
    assert np.array_equal(_bits(dense), _want_bits(W.reference_f64(p, [45], [0.5])))
