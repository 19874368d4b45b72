"""CPU: the helpers of tests/_rotations.py, and the input precondition of the NV quantizer fuzz.  That fuzz (tests/test_gpu_rotation_orientation.py) allows the device
a few scale bytes and codes off the oracle because the order of the rotation's fp32 sums is free; the caps are therefore a condition on the INPUTS as much as on the
kernel: for the very same draws the oracle under its two accumulation models (a k-ascending fp32 fma chain, and the exact sum rounded once) must disagree in at most
half of each cap.  A draw that did not would have to be changed -- never the cap."""
import numpy as np
import pytest
import torch

import oracle
import _rotations as rot


@pytest.mark.parametrize("R", [16, 32, 64, 128])
def test_signed_permuted_hadamard_is_orthogonal_and_not_symmetric(R):
    h = rot.signed_permuted_hadamard(R, seed=3)           # (the helper asserts h != h.T and h @ h.T == I itself)
    assert h.dtype == torch.bfloat16 and h.shape == (R, R)
    assert (h != h.T).float().mean() > 0.25
    assert torch.equal(h, rot.signed_permuted_hadamard(R, seed=3)) and not torch.equal(h, rot.signed_permuted_hadamard(R, seed=4))
    g = rot.general_rotation(R, seed=3)
    assert g.shape == (R, R) and not torch.equal(g, g.T.contiguous())


@pytest.mark.parametrize("fmt,R", [("mx", 32), ("mx", 64), ("mx", 128), ("nv", 16), ("nv", 32), ("nv", 64), ("nv", 128)])
@pytest.mark.parametrize("method", [oracle.QUEST, oracle.ABS_MAX])
def test_exact_regime_has_zero_tolerance_and_sees_a_transposed_rotation(fmt, R, method):
    """x = 100 x integers in -2 .. 2 and a +-c rotation: the oracle's two accumulation models give the same bytes (every product and sum is exact), and rotating by h.T
    instead changes most of the codes -- the zero-tolerance comparisons of tests/test_gpu_rotation_orientation.py can tell the two orientations apart."""
    h = rot.bits(rot.signed_permuted_hadamard(R, seed=1))
    x = rot.bits(rot.exact_input((70, 3 * max(R, 32)), seed=R))
    run = (lambda hh, acc: oracle.fused_quantize_mx(x, hh, method, acc_model=acc)[:2]) if fmt == "mx" else (lambda hh, acc: oracle.fused_quantize_nv(x, hh, 2.3, method, acc_model=acc))
    (q0, s0), (q1, s1), (qt, st) = run(h, 0), run(h, 1), run(np.ascontiguousarray(h.T), 1)
    assert np.array_equal(q0, q1) and np.array_equal(s0, s1)
    assert (~oracle.codes_equal_mod_zero_sign(qt, q1)).mean() > 0.5


def test_nv_fuzz_draws_meet_the_caps_with_margin():
    seen_r, seen_general = set(), 0
    for it, R, x, h, gs, method in rot.nv_fuzz_draws():
        assert not torch.equal(h, h.T.contiguous())
        m = oracle.QUEST if method == "quest" else oracle.ABS_MAX
        q0, s0 = oracle.fused_quantize_nv(rot.bits(x), rot.bits(h), gs, m, acc_model=0)
        q1, s1 = oracle.fused_quantize_nv(rot.bits(x), rot.bits(h), gs, m, acc_model=1)
        cap_s, cap_c = rot.nv_fuzz_caps(s1.size, 2 * q1.size)
        sbad = int((s0 != s1).sum())
        cbad = int((~oracle.codes_equal_mod_zero_sign(q0, q1) & (s0 == s1).repeat(16)).sum())
        assert sbad <= cap_s / 2 and cbad <= cap_c / 2, (it, R, method, tuple(x.shape), sbad, cap_s, cbad, cap_c)
        seen_r.add(R)
        seen_general += it % 2
    assert seen_r == {16, 32, 64, 128} and seen_general == rot.NV_FUZZ_ITERS // 2
