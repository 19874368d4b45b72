"""CPU: the bound of tests/test_gpu_moe_layer_vs_fp64.py CAN fail.  That test accepts a device layer within 0.25 x |L_q - L_fp64| of the oracle-quantized model L_q
(tests/_moe_model.py); here, without a GPU, every convention error the bound is there to catch is applied to the model itself and must move it by at least 1.0 x that
noise -- four times the bound: the activations rotated by h.T, the two routing weights of a token exchanged, the gate and up halves exchanged, and (NV) the neighbouring
expert's a2 global scale in the second quantizer.  Also the preconditions the GPU test relies on: neighbouring router scores at least 1e-3 apart in fp64 (ids can be
compared exactly), one expert empty, and the oracle's two accumulation models within 0.01 x noise of each other (summation order does not move a correct result).

Quantization noise |L_q - L_fp64| / |L_fp64| of the three layers (T 33, E 8, topk 2, H = I 256):  mx_abs_max (R 32, alpha 1/9) 0.290;  mx_quest (R 64, alpha 1) 0.396;
nv_grouped (R 32, per-expert global scales, alpha 1 / (gs_a gs_w)) 0.238.  Distances of the wrong variants from L_q in units of the noise, in the order above:
mx_abs_max 4.85 / 1.87 / 3.31;  mx_quest 2.66 / 1.20 / 1.90;  nv_grouped 5.83 / 1.20 / 4.10 / 20.3."""
import functools

import numpy as np
import pytest

import _moe_model as mm


@functools.lru_cache(maxsize=None)
def _case(name):
    layer = mm.make_layer(name)
    ids, weights, gap = mm.route_fp64(layer)
    wq = mm.quantize_weights(layer)
    l_fp64 = mm.layer_fp64(layer, ids, weights)
    l_q = mm.layer_quantized(layer, ids, weights, wq)
    return layer, ids, weights, gap, wq, l_fp64, l_q, mm.fro(l_q - l_fp64)


@pytest.fixture(scope="module", params=list(mm.LAYERS))
def case(request):
    return _case(request.param)


def test_router_scores_are_well_separated_and_one_expert_is_empty(case):
    layer, ids, weights, gap, *_ = case
    assert gap > mm.MIN_GAP, gap
    counts = np.bincount(ids.reshape(-1), minlength=mm.E)
    assert counts[mm.EMPTY] == 0 and (np.delete(counts, mm.EMPTY) > 0).all() and counts.sum() == mm.T * mm.TOPK, counts
    assert (ids[:, 0] != ids[:, 1]).all() and np.allclose(weights.sum(axis=1), 1.0)
    assert (np.abs(weights[:, 0] - weights[:, 1]) > 1e-2).mean() > 0.9   # exchanging a token's two weights changes something


def test_layer_shapes_and_scales(case):
    layer = case[0]
    assert not np.array_equal(layer.h, layer.h.T)
    if layer.fmt == "nv":
        s = np.concatenate([layer.a13_gs, layer.a2_gs, layer.w13_gs, layer.w2_gs])
        assert len(np.unique(s)) == 4 * mm.E and ((s.view(np.uint32) & 0x7fffff) != 0).all()
        assert layer.alpha13.shape == (mm.E,) and np.array_equal(layer.alpha2, (1.0 / (layer.a2_gs * layer.w2_gs)).astype(np.float32))
    else:
        assert float(layer.alpha13[0]) == float(np.float32(1.0 / 9.0 if layer.method == "abs_max" else 1.0))


def test_quantization_noise_is_what_fp4_gives(case):
    layer, *_, l_fp64, l_q, noise = case
    rel = noise / mm.fro(l_fp64)
    print(f"{layer.name}: |L_q - L_fp64| / |L_fp64| = {rel:.4f}")
    assert np.isfinite(l_q).all() and 0.1 < rel < 0.5, rel    # two fp4 GEMMs in a row: tens of percent, and a wrong alpha (9, 1 / 3, a missing global scale) is far outside


def test_accumulation_order_does_not_move_the_layer(case):
    layer, ids, weights, _, _, _, l_q, noise = case
    l_q0 = mm.layer_quantized(layer, ids, weights, mm.quantize_weights(layer, acc_model=0), acc_model=0)
    assert mm.fro(l_q0 - l_q) <= 0.01 * noise, mm.fro(l_q0 - l_q) / noise


def test_the_neighbours_global_scale_lies_far_outside_the_bound():
    layer, ids, weights, _, wq, _, l_q, noise = _case("nv_grouped")   # (MX has no global scale)
    d = mm.fro(mm.layer_quantized(layer, ids, weights, wq, neighbour_a2=True) - l_q) / noise
    print(f"{layer.name} neighbour_a2: {d:.2f} x noise")
    assert d >= 1.0, d


@pytest.mark.parametrize("variant", ["ha", "swap_weights", "swap_gate_up"])
def test_a_wrong_convention_lies_far_outside_the_bound(case, variant):
    layer, ids, weights, _, wq, _, l_q, noise = case
    kw = {"ha": layer.h.T} if variant == "ha" else {variant: True}
    d = mm.fro(mm.layer_quantized(layer, ids, weights, wq, **kw) - l_q) / noise
    print(f"{layer.name} {variant}: {d:.2f} x noise")
    assert d >= 1.0, d
