"""CPU: the bound of tests/test_gpu_moe_layer_vs_fp64.py CAN fail.  That test accepts a device layer within 0.25 x |L_q - L_fp64| of the oracle-quantized model L_q
(tests/_moe_model.py); here, without a GPU, every convention error the bound is there to catch is applied to the model itself and must move it by at least 1.0 x that
noise -- four times the bound: the activations rotated by h.T, the two routing weights of a token exchanged, the gate and up halves exchanged, and (NV) the neighbouring
expert's a2 global scale in the second quantizer.  Also the preconditions the GPU test relies on: neighbouring router scores at least 1e-3 apart in fp64 (ids can be
compared exactly), one expert empty, and the oracle's two accumulation models within 0.01 x noise of each other (summation order does not move a correct result).

Quantization noise |L_q - L_fp64| / |L_fp64| of the three layers (T 33, E 8, topk 2, H = I 256):  mx_abs_max (R 32, alpha 1/9) 0.290;  mx_quest (R 64, alpha 1) 0.396;
nv_grouped (R 32, per-expert global scales, alpha 1 / (gs_a gs_w)) 0.238.  Distances of the wrong variants from L_q in units of the noise, in the order above:
mx_abs_max 4.85 / 1.87 / 3.31;  mx_quest 2.66 / 1.20 / 1.90;  nv_grouped 5.83 / 1.20 / 4.10 / 20.3.

The four layers of tests/_moe_model_more.py, the same sizes (for the MXFP8 quantizers the two accumulation models are the fp64 rotation rounded to fp32 and a sequential
fp32 sum; all four lie 0.0 x noise apart -- mxf8_silu's seed is one at which the two models give the same WEIGHT bytes, asserted below: three near-tie codes among
1.5 M weights moved another seed's layer by 0.023 x noise).  Noise / |L_fp64| and the distances in noise units:

  mxf8_silu (e4m3, R 32, alpha 1)              0.0668   h.T 20.8, weights exchanged 9.17, halves exchanged 14.7, e5m2's scale shift 14.9
  oai_mx (MXFP4 abs_max, R 64, alpha 1/9)      0.2332   h.T 5.15, weights exchanged 2.82, halves exchanged 3.36, left interleaved 5.34, odd rows as gate 2.96, neighbour's
                                                        b1 2.99, neighbour's b2 2.92, b2 unweighted 2.19, no clamp 1.76, no + 1 1.15        (alpha 1.0: 0.34 -- NOT caught)
  oai_w4a8 (checkpoint bytes, identity, R 32)  0.0479   weights exchanged 11.2, halves exchanged 17.3, left interleaved 28.5, odd rows as gate 16.0, neighbour's b1 12.3,
                                                        neighbour's b2 7.09, b2 unweighted 5.50, no clamp 24.9, no + 1 4.15, nibbles exchanged 28.1, scales (E, K/32, N)
                                                        22.8                                                                                  (alpha 1.0: 0.57 -- NOT caught)
  oai_w4a8_ep rank 0 / rank 1                  0.0486 / 0.0468   the same flags 4.08 ... 29.4 on either rank (the least: no + 1, 4.08 / 4.32); on rank 1 rank 0's stacks
                                                        30.5 and the global expert index into b1 / b2 13.6 (on rank 0 global and local indices coincide: 0)

The W4A8 noise is a fifth of the FP4 layers': the checkpoint's weights ARE the fp64 weights, only the e4m3 activations are rounded.  The sigmoid's alpha (1.0 for 1.702)
stays below 1.0 x noise in both gpt-oss layers -- gates clamped at 7 or strongly negative saturate the sigmoid whatever alpha is -- so the layer test does not claim it:
tests/test_gpu_swiglu_oai.py pins alpha bit for bit against the numpy model, for both values.  The data that makes the rest visible is asserted below: gate/up weights
of rms 0.28 ... 0.42 put 12 ... 15 % of the routed gates above the limit and 6 ... 30 % of the ups outside it, and both biases are of the size of what they meet."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import pytest

import _moe_model as mm
import _moe_model_more as more
import _swiglu_oai_model as oai
import oracle


class Case(NamedTuple):
    layer: object
    rank: Optional[int]     # the expert-parallel layer: the rank whose partial is judged
    kw: dict                # {"rank": rank} or {}
    ids: np.ndarray
    weights: np.ndarray
    gap: float
    wq: object              # the uploaded weights (of the rank)
    l_fp64: np.ndarray
    l_q: np.ndarray
    noise: float


@functools.lru_cache(maxsize=None)
def _routed(name):
    layer = mm.make_layer(name)
    return (layer,) + tuple(mm.route_fp64(layer)) + (mm.quantize_weights(layer),)


def _stacks(case_or_rank, wq):
    rank = case_or_rank.rank if isinstance(case_or_rank, Case) else case_or_rank
    return wq if rank is None else more.rank_stacks(wq, rank)


@functools.lru_cache(maxsize=None)
def _case(name, rank=None):
    layer, ids, weights, gap, wq = _routed(name)
    kw = {} if rank is None else {"rank": rank}
    wq = _stacks(rank, wq)
    l_fp64 = mm.layer_fp64(layer, ids, weights, **kw)
    l_q = mm.layer_quantized(layer, ids, weights, wq, **kw)
    return Case(layer, rank, kw, ids, weights, gap, wq, l_fp64, l_q, mm.fro(l_q - l_fp64))


MORE = [("mxf8_silu", None), ("oai_mx", None), ("oai_w4a8", None), ("oai_w4a8_ep", 0), ("oai_w4a8_ep", 1)]
_id = lambda p: p[0] if p[1] is None else f"{p[0]}-rank{p[1]}"


@pytest.fixture(scope="module", params=[(n, None) for n in mm.LAYERS] + MORE, ids=_id)
def case(request):
    return _case(*request.param)


@pytest.fixture(scope="module", params=[(n, None) for n in mm.LAYERS] + [p for p in MORE if mm.make_layer(p[0]).fmt == "mx"], ids=_id)
def fp4_case(request):
    return _case(*request.param)


@pytest.fixture(scope="module", params=[p for p in MORE if mm.make_layer(p[0]).fmt != "mx"], ids=_id)
def e4m3_case(request):
    return _case(*request.param)


@pytest.fixture(scope="module", params=[p for p in MORE if mm.make_layer(p[0]).kind == "oai"], ids=_id)
def oai_case(request):
    return _case(*request.param)


def _distance(c: Case, wq=None, **wrong) -> float:
    return mm.fro(mm.layer_quantized(c.layer, c.ids, c.weights, c.wq if wq is None else wq, **c.kw, **wrong) - c.l_q) / c.noise


def test_router_scores_are_well_separated_and_one_expert_is_empty(case):
    ids, weights = case.ids, case.weights
    assert case.gap > mm.MIN_GAP, case.gap
    counts = np.bincount(ids.reshape(-1), minlength=mm.E)
    assert counts[mm.EMPTY] == 0 and (np.delete(counts, mm.EMPTY) > 0).all() and counts.sum() == mm.T * mm.TOPK, counts
    assert (ids[:, 0] != ids[:, 1]).all() and np.allclose(weights.sum(axis=1), 1.0)
    assert (np.abs(weights[:, 0] - weights[:, 1]) > 1e-2).mean() > 0.9   # exchanging a token's two weights changes something


def test_layer_shapes_and_scales(case):
    layer = case.layer
    if layer.fmt == "w4a8":
        assert np.array_equal(oai.bf16_to_f64(layer.h), np.eye(layer.rot))
    else:
        assert not np.array_equal(layer.h, layer.h.T)
    if layer.fmt == "nv":
        s = np.concatenate([layer.a13_gs, layer.a2_gs, layer.w13_gs, layer.w2_gs])
        assert len(np.unique(s)) == 4 * mm.E and ((s.view(np.uint32) & 0x7fffff) != 0).all()
        assert layer.alpha13.shape == (mm.E,) and np.array_equal(layer.alpha2, (1.0 / (layer.a2_gs * layer.w2_gs)).astype(np.float32))
    else:
        nine = layer.fmt == "mx" and layer.method == "abs_max"    # only MXFP4 abs_max stores codes at 3 x the value
        assert float(layer.alpha13[0]) == float(layer.alpha2[0]) == float(np.float32(1.0 / 9.0 if nine else 1.0))


def _print_noise(c: Case) -> float:
    rel = c.noise / mm.fro(c.l_fp64)
    print(f"{c.layer.name} {c.kw}: |L_q - L_fp64| / |L_fp64| = {rel:.4f}")
    assert np.isfinite(c.l_q).all()
    return rel


def test_quantization_noise_is_what_fp4_gives(fp4_case):
    rel = _print_noise(fp4_case)
    assert 0.1 < rel < 0.5, rel    # two fp4 GEMMs in a row: tens of percent, and a wrong alpha (9, 1 / 3, a missing global scale) is far outside


def test_quantization_noise_is_what_e4m3_gives(e4m3_case):
    """e4m3 keeps four significant bits: a rounding error of about 2^-4 / sqrt(3) / 1.4 = 0.026 rms per operand, two to four quantized operands and two GEMMs in a
    row -- some percent.  An fp4-sized noise, a scale off by a power of two or e5m2's shift (saturated codes) are far outside"""
    rel = _print_noise(e4m3_case)
    assert 0.02 < rel < 0.12, rel


def test_accumulation_order_does_not_move_the_layer(case):
    layer = case.layer
    wq0 = _stacks(case, mm.quantize_weights(layer, acc_model=0))
    if layer.fmt == "mxf8":   # (the data is chosen so: the weights a deployment uploads do not depend on how its quantizer summed)
        assert all(np.array_equal(a, b) for a, b in zip(wq0[:4], case.wq[:4]))
    l_q0 = mm.layer_quantized(layer, case.ids, case.weights, wq0, acc_model=0, **case.kw)
    assert mm.fro(l_q0 - case.l_q) <= 0.01 * case.noise, mm.fro(l_q0 - case.l_q) / case.noise


def test_the_neighbours_global_scale_lies_far_outside_the_bound():
    c = _case("nv_grouped")   # (MX has no global scale)
    d = _distance(c, neighbour_a2=True)
    print(f"{c.layer.name} neighbour_a2: {d:.2f} x noise")
    assert d >= 1.0, d


def _applies(p, variant) -> bool:
    """which wrong variant can be built on which layer: h.T needs a rotation that is not the identity, the rest their format or activation"""
    if p[0] in mm.LAYERS:
        return variant in ("ha", "swap_weights", "swap_gate_up")
    kind, fmt = more.LAYERS[p[0]][:2]
    return {"ha": fmt != "w4a8", "swap_weights": True, "swap_gate_up": True, "e5m2_shift": fmt == "mxf8", "swap_nibbles": fmt == "w4a8",
            "scales_kn": fmt == "w4a8"}.get(variant, kind == "oai")


def _wrong(layers, variants):
    return pytest.mark.parametrize("case,variant", [pytest.param(p, v, id=f"{_id(p)}-{v}") for p in layers for v in variants if _applies(p, v)], indirect=["case"])


@_wrong([(n, None) for n in mm.LAYERS] + MORE, ["ha", "swap_weights", "swap_gate_up"])
def test_a_wrong_convention_lies_far_outside_the_bound(case, variant):
    layer = case.layer
    d = _distance(case, **({"ha": layer.h.T} if variant == "ha" else {variant: True}))
    print(f"{layer.name} {case.kw} {variant}: {d:.2f} x noise")
    assert d >= 1.0, d


# ---- the MXFP8, gpt-oss and W4A8 layers: their own conventions -------------------------------------------------------------------------------------------------------
def _routed_gate_up(c: Case):
    """the fp64 gate and up values (bias added) of every routed slot, (T topk, I) each"""
    layer = c.layer
    w13, _ = more.weights_fp64(layer)
    x = oai.bf16_to_f64(layer.tok)
    gu = np.stack([w13[e] @ x[t] + oai.bf16_to_f64(layer.b1[e]) for t in range(mm.T) for e in c.ids[t]])
    return gu[:, 0::2], gu[:, 1::2]


def test_gpt_oss_data_makes_the_conventions_visible(oai_case):
    c, layer = oai_case, oai_case.layer
    g, u = _routed_gate_up(c)
    over_g, over_u = float((g > more.LIMIT).mean()), float((np.abs(u) > more.LIMIT).mean())
    print(f"{layer.name}: gate above the limit {over_g:.3f}, up outside it {over_u:.3f}")
    assert 0.08 < over_g < 0.3 and 0.04 < over_u < 0.4          # the clamp acts on both, and most elements stay inside it
    b1, b2 = oai.bf16_to_f64(layer.b1), oai.bf16_to_f64(layer.b2)
    assert 0.2 < b1.std() / np.concatenate([g, u]).std() < 1.0  # b1 against what it is added to
    _, w2 = more.weights_fp64(layer)
    full = _case(layer.name, None) if c.rank is not None else c
    y_rms = mm.fro(full.l_fp64) / np.sqrt(full.l_fp64.size)
    assert 0.1 < b2.std() / y_rms < 1.0                         # b2 against the layer's output
    # neighbouring experts' biases have nothing in common, so taking the neighbour's is a different layer
    for b in (b1, b2):
        assert all(abs(np.corrcoef(b[e], b[(e + 1) % mm.E])[0, 1]) < 0.25 for e in range(mm.E))


def test_w4a8_checkpoint_bytes_mean_what_the_oracle_says():
    """the fp64 weight of L_fp64 (tests/_w4a8_model.py's tables) is the oracle's dequantization of the same bytes: nibble order and scale rule agree between the judges"""
    ck = mm.make_layer("oai_w4a8").ck
    for c, s in ((ck["w13c"], ck["w13s"]), (ck["w2c"], ck["w2s"])):
        assert np.array_equal(more.dequant_e2m1(c[0], s[0]), oracle.dequant_fp4(c[0], s[0], 32, False).reshape(c.shape[1], -1).astype(np.float64))
        assert len(np.unique(s)) >= 4 and len(np.unique(c)) == 256     # exchanging nibbles or misplacing scales changes the weights


def test_the_ranks_partials_sum_to_the_unsplit_layer():
    full, r0, r1 = _case("oai_w4a8"), _case("oai_w4a8_ep", 0), _case("oai_w4a8_ep", 1)
    for f in ("tok", "logits", "b1", "b2"):
        assert np.array_equal(getattr(full.layer, f), getattr(r0.layer, f))
    assert np.array_equal(full.ids, r0.ids) and mm.fro(r0.l_fp64) > 0 and mm.fro(r1.l_fp64) > 0
    assert np.abs(r0.l_fp64 + r1.l_fp64 - full.l_fp64).max() <= 1e-12 * np.abs(full.l_fp64).max()
    # every rank has work and dropped slots, and tokens with one slot on each rank exist: pos -1 next to a real row
    on0 = full.ids < mm.E // more.RANKS
    assert on0.any(axis=1).sum() > 5 and (~on0).any(axis=1).sum() > 5 and (on0[:, 0] != on0[:, 1]).sum() > 5
    assert np.array_equal(more.expert_map(0), [0, 1, 2, 3, -1, -1, -1, -1]) and np.array_equal(more.expert_map(1), [-1, -1, -1, -1, 0, 1, 2, 3])


OAI_WRONG = ["neighbour_b1", "neighbour_b2", "unweighted_b2", "no_clamp", "no_plus_one"]
OAI_WRONG_UPLOAD = ["no_split", "odd_gate"]
W4A8_WRONG_UPLOAD = ["swap_nibbles", "scales_kn"]


@_wrong(MORE, OAI_WRONG + OAI_WRONG_UPLOAD + W4A8_WRONG_UPLOAD + ["e5m2_shift"])
def test_a_wrong_convention_of_the_new_layers_lies_far_outside_the_bound(case, variant):
    c, layer = case, case.layer
    if variant in OAI_WRONG_UPLOAD + W4A8_WRONG_UPLOAD:
        d = _distance(c, wq=_stacks(c, mm.quantize_weights(layer, **{variant: True})))
    else:
        d = _distance(c, **{variant: True})
    print(f"{layer.name} {c.kw} {variant}: {d:.2f} x noise")
    assert d >= 1.0, d


def test_expert_parallel_mistakes_lie_far_outside_the_bound():
    c = _case("oai_w4a8_ep", 1)
    full = _routed("oai_w4a8_ep")[4]
    d_stacks = _distance(c, wq=more.rank_stacks(full, 0))     # rank 1 computing with rank 0's weights and biases
    d_index = _distance(c, global_bias_index=True)            # b1 / b2 addressed by the global expert index
    print(f"oai_w4a8_ep rank 1: rank 0's stacks {d_stacks:.2f}, global bias index {d_index:.2f} x noise")
    assert d_stacks >= 1.0 and d_index >= 1.0, (d_stacks, d_index)
    assert _distance(_case("oai_w4a8_ep", 0), global_bias_index=True) == 0.0   # on rank 0 the two indices coincide: only rank 1 can show it


@pytest.mark.parametrize("name", ["oai_mx", "oai_w4a8"])
def test_alpha_is_not_claimed_by_the_layer_bound(name):
    """alpha 1.0 for 1.702 moves the layers by less than the 1.0 x noise this file asks of a caught mistake (saturated gates hide it): recorded, not claimed --
    tests/test_gpu_swiglu_oai.py compares the op with the numpy model bit for bit at both alphas"""
    d = _distance(_case(name), alpha_one=True)
    print(f"{name} alpha_one: {d:.2f} x noise")
    assert d > 0.0
