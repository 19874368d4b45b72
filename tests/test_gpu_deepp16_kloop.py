"""The K-loop forms of the one-tile 16x16x128 MXFP4 kernel (csrc/gemm_mx_deepp16.hip.h, KL_ bits), through the lab library with the form forced.

"gemm_variant" 192 = the loop before the forms existed, 193 = KL_SCALES (K-blocks interleaved across a stage's two MFMAs, the lane's two scale bytes in one register,
byte select 0 / 1), 194 = KL_DMA (one statement per LDS-DMA piece from loop-invariant offsets in the stages that fetch neither the K tail nor past the end),
195 = both, 196 = both with the pieces spread over the whole of half 1, 197 = KL_DMA with the pieces spread; 191 = whichever of them the product launches.

  block pairing   A's codes are zero outside K-block j of every stage, B is dense, the scale bytes of the 8 blocks of a stage are distinct in both operands and so is
                  their sum: a lane that takes another block's data loses the block, one that takes another block's scale byte (of either operand, or of both) is
                  off by a power of two.  256 x 256 x 1536 is six stages, the smallest K whose launch runs a pair of KL_DMA stages; x 512 is prologue + last stage.
  K tails         K = 512 - 32 t, t = 1 ... 7 at 257 x 264, the operands embedded in 0xFF bytes: the op takes K % 128 == 0, so t = 4 is the one tail length that
                  exists inside the interleaved last stage (half of it); the other six are refused by the entry.  K = 1920 puts the same tail behind the KL_DMA pairs.
  old against new every form against 192 on the shapes of tests/test_gpu_deepp16.py: equal bytes.

Operands, oracle references and the guarded call are those of tests/_mx_cases.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mx_cases as mc  # noqa: E402

OLD, PRODUCT = 192, 191
FORMS = [193, 194, 195, 196, 197]
SHAPES = [(256, 256, 512), (256, 256, 1024), (512, 768, 1536), (257, 264, 896), (1, 8, 512), (1280, 2048, 512)]   # those of tests/test_gpu_deepp16.py
PAIRING_SHAPES = [(256, 256, 1536), (256, 256, 512)]


def _case(variant, shape):
    return mc.Case("mxf4", False, variant, (), *shape)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd  # noqa: F401


def test_the_shapes_reach_the_loops_they_are_meant_for():
    """the one-tile kernel's K walk: stage 0, pairs of KL_DMA stages while kt + 4 < KT (kt = 1, 3, ...), the masked stages, the last stage"""
    lean = lambda k: len(range(1, max(-(-(k // 2) // 128) - 4, 1), 2))   # noqa: E731
    assert lean(1536) == 1 and lean(1024) == 0 and lean(512) == 0
    for m, n, k in PAIRING_SHAPES + [(257, 264, 512 - 32 * t) for t in range(1, 8)]:
        kt = -(-(k // 2) // 128)
        assert -(-m // 256) * -(-n // 256) <= 256 and kt % 2 == 0


@functools.lru_cache(maxsize=None)
def _pairing_data(shape, j):
    m, n, k = shape
    c = _case(0, shape)
    rng = np.random.default_rng(1000 * k + j)
    kb = k // 32
    g8 = np.arange(kb) % 8
    a = rng.integers(0, 256, size=(m, k // 2), dtype=np.uint8)
    a.reshape(m, kb, 16)[:, g8 != j, :] = 0
    b = rng.integers(0, 256, size=(n, k // 2), dtype=np.uint8)
    ra, rb = np.arange(mc.pad128(m))[:, None], np.arange(mc.pad128(n))[:, None]
    # block g of a stage: A byte 118 + g + u(r), B byte 121 + 2 g + v(c), u, v in {0, 1}: 8 distinct bytes per operand and 8 distinct sums 239 + 3 g (2^-15 ... 2^6)
    sa = (118 + g8[None, :] + (ra * 7 + ra // 16) % 2).astype(np.uint8)
    sb = (121 + 2 * g8[None, :] + (rb * 5 + rb // 16) % 2).astype(np.uint8)
    assert len(set(sa[0, :8])) == 8 and len(set(sb[0, :8])) == 8 and len(set((sa[0, :8].astype(int) + sb[0, :8]))) == 8
    return mc.Data(a, b, sa, sb, mc._reference(c, a, b, sa, sb, 1.0), 1.0)


@pytest.mark.parametrize("shape", PAIRING_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", FORMS + [PRODUCT])
def test_block_pairing(form, shape):
    for j in range(8):
        d = _pairing_data(shape, j)
        assert d.ref.any(), "the reference of a pairing case is all zero"
        r = mc.run(_case(form, shape), d)
        mc.assert_footprint(r)
        mc.assert_equals_reference(r.out, d.ref)
        assert not mc.isnan_bf16(r.out).any()


@pytest.mark.parametrize("t", range(1, 8))
def test_k_tails_inside_the_interleaved_last_stage(t):
    """K = 512 - 32 t.  matmul_mxf4_bf16_tn takes K % 128 == 0 only (the reference's contract), so of these seven only t = 4 (K = 384: the last stage's K-blocks 4 ... 7
    missing, i.e. lane groups 2 and 3 of BOTH its MFMAs) is a K the op runs; the other six must be refused by the entry before anything is launched."""
    shape = (257, 264, 512 - 32 * t)
    if shape[2] % 128:
        c = _case(PRODUCT, shape)
        d = mc.Data(np.zeros((257, shape[2] // 2), np.uint8), np.zeros((264, shape[2] // 2), np.uint8), np.zeros((384, shape[2] // 32), np.uint8),
                    np.zeros((384, shape[2] // 32), np.uint8), None, 1.0)
        with pytest.raises(AssertionError, match="K must be a positive multiple of 128"):
            mc.run(c, d, fill=0xFF)
        return
    _tail(shape)


def test_k_tail_fetched_by_a_masked_stage_behind_the_kl_dma_pairs():
    """K = 1920: 7.5 stages -- two pairs of KL_DMA stages, then the masked stage that fetches the half-filled last stage"""
    _tail((257, 264, 1920))


def _tail(shape):
    d = mc.dataset(_case(0, shape), "plain")
    for form in FORMS + [PRODUCT]:
        r = mc.run(_case(form, shape), d, fill=0xFF)
        mc.assert_footprint(r)
        mc.assert_equals_reference(r.out, d.ref)
        assert not mc.isnan_bf16(r.out).any(), form


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_form_equals_the_loop_it_replaces(shape):
    d = mc.dataset(_case(0, shape), "plain")
    old = mc.run(_case(OLD, shape), d)
    mc.assert_footprint(old)
    mc.assert_equals_reference(old.out, d.ref)
    for form in FORMS + [PRODUCT]:
        r = mc.run(_case(form, shape), d)
        mc.assert_footprint(r)
        assert np.array_equal(r.out, old.out), f"form {form}: {int((r.out != old.out).sum())} outputs differ from the loop it replaces"
