"""Rotation matrices that are NOT their own transpose, and the exact-arithmetic input that goes with them -- shared by the tests that pin which way round
the rotate-and-quantize ops apply h (y = x_group @ h, oracle/qutlass_oracle.c rotate_group; never h.T).  The Sylvester matrix of every `_hadamard(n)` helper in
tests/ equals its transpose, so a kernel that applied h.T on one of its staging paths would pass every test built on it.  Plain module: numpy and torch on the CPU."""
import numpy as np
import torch


def _sylvester(n: int) -> np.ndarray:
    h = np.ones((1, 1), dtype=np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == n, n
    return h


def signed_permuted_hadamard(R: int, seed: int = 0) -> torch.Tensor:
    """h = (P H D) R^-0.5 as (R, R) bf16 on the CPU: H the Sylvester matrix, P a random row permutation, D a random +-1 diagonal.  Orthogonal, every entry of one
    magnitude (so the exact regime of `exact_input` holds as it does for H itself), and far from symmetric: transposing it changes about half of its entries."""
    rng = np.random.default_rng(1000 * R + seed)
    while True:
        s = _sylvester(R)[rng.permutation(R)] * rng.choice([-1, 1], size=R)[None, :]
        if (s != s.T).mean() >= 0.25:
            break
    assert (s != s.T).any(), "the rotation must differ from its transpose"
    assert np.array_equal(s @ s.T, R * np.eye(R, dtype=np.int64)), "the rotation must be orthogonal: h @ h.T == I"
    h = torch.from_numpy(s.astype(np.float32) * np.float32(R ** -0.5)).to(torch.bfloat16)
    assert not torch.equal(h, h.T.contiguous())
    # after rounding to bf16 every entry is +-c for ONE c: h @ h.T == (R c^2) I exactly, the identity up to bf16's rounding of R^-0.5
    c = float(h.abs().max())
    assert torch.equal(h.abs().float(), torch.full((R, R), c)) and abs(R * c * c - 1.0) < 2.0 ** -7
    assert torch.equal(h.double() @ h.double().T, R * c * c * torch.eye(R, dtype=torch.float64))
    return h


def general_rotation(R: int, seed: int = 0) -> torch.Tensor:
    """0.2 * randn(R, R) as bf16: no structure at all (neither orthogonal nor symmetric), as in the MX golden fixture's random case"""
    gen = torch.Generator(device="cpu").manual_seed(7000 + 10 * R + seed)
    h = (torch.randn(R, R, generator=gen) * 0.2).to(torch.bfloat16)
    assert not torch.equal(h, h.T.contiguous())
    return h


def exact_input(shape, seed: int, scale: float = 100.0) -> torch.Tensor:
    """Integers in -2 .. 2 times 100 (scale) as bf16 on the CPU: with a rotation whose entries are all +-c every product x * h is an integer multiple of 100 c below 2^9 of
    them, and every partial sum of up to 128 products in any order is exact in fp32 -- the oracle and any kernel must agree to the bit, the tolerance is zero."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(-2, 3, tuple(shape), generator=gen).float() * scale).to(torch.bfloat16)


def bits(t: torch.Tensor) -> np.ndarray:
    """torch tensor -> numpy for the oracle: bf16 as uint16 bit patterns, one-byte types as uint8"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.uint16).numpy()
    if t.element_size() == 1:
        return t.view(torch.uint8).numpy()
    return t.numpy()


NV_FUZZ_ITERS = 24


def nv_fuzz_draws():
    """The draws of the NV quantizer fuzz (tests/test_gpu_rotation_orientation.py) -- one generator, so that tests/test_rotations_cpu.py can show for the very same
    inputs that the test's caps hold with margin between the oracle's two accumulation models.  Mirrors the MX half of test_fuzz_quantizers_and_swizzle: R of
    16 / 32 / 64 / 128, up to two leading dimensions, 1 .. 39 rows, 1 .. 5 rotation widths of columns, magnitudes 0.01 / 1 / 25 / 3000, a random global scale, both
    methods; every second iteration (the odd ones) rotates by a general random matrix, the others by a signed, row-permuted Hadamard matrix -- never a symmetric h.
    Yields (it, R, x bf16 CPU tensor, h (R, R) bf16 CPU tensor, global_scale float, method)."""
    rng = np.random.default_rng(109)
    for it in range(NV_FUZZ_ITERS):
        R = int(rng.choice([16, 32, 64, 128]))
        lead = tuple(int(v) for v in rng.integers(1, 5, size=int(rng.integers(0, 3))))
        rows, cols = int(rng.integers(1, 40)), int(rng.integers(1, 6)) * max(R, 32)
        mag = float(rng.choice([0.01, 1.0, 25.0, 3000.0]))
        x = torch.from_numpy(rng.standard_normal(lead + (rows, cols)).astype(np.float32) * mag).to(torch.bfloat16)
        gs = float(np.float32(rng.uniform(0.3, 8.0)))
        method = str(rng.choice(["quest", "abs_max"]))
        h = general_rotation(R, seed=it) if it % 2 else signed_permuted_hadamard(R, seed=it)
        yield it, R, x, h, gs, method


def nv_fuzz_caps(n_scales: int, n_codes: int):
    """test_fuzz_quantizers_and_swizzle's caps: scale bytes differing, codes differing within the groups whose scale agrees"""
    return max(1, 2e-3 * n_scales), max(2, 2e-3 * n_codes)
