"""The MXFP6 rotate-and-quantize ops on the GPU -- fusedQuantizeMxf6, fusedGatherQuantizeMxf6 -- byte for byte against the numpy model of their contract
(tests/_mxf6_model.py, pinned by tests/test_mxf6_model_cpu.py), on inputs whose y = x_group @ h is exact: the identity rotation, and tests/_rotations' exact inputs
with a non-symmetric rotation.

A wave owns a tile of 32 rows x max(R, 32) elements and a workgroup has 4 waves: the shapes (1, 128), (33, 256), (70, 640) cover less than a tile, a tile's tail
and more than one workgroup."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mxf6_model as model  # noqa: E402
import _rotations as rot  # noqa: E402
from _rotations import bits as _np  # noqa: E402

DEV = "cuda:0"
ROTS = (32, 64, 128)
SHAPES = ((1, 128), (33, 256), (70, 640))


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _identity(R):
    return torch.eye(R, dtype=torch.bfloat16)


def _flat(sf, n):
    return _np(sf).reshape(-1)[:n]


def _run(q, x, h):
    """the plain op on CPU tensors -> (packed codes uint8 (.., 3K/4), the numel / 32 flat scale bytes)"""
    codes, sf = q.fusedQuantizeMxf6(x.to(DEV), h.to(DEV))
    assert codes.dtype == torch.uint8 and codes.shape == (*x.shape[:-1], x.shape[-1] * 3 // 4) and sf.dtype == torch.float8_e8m0fnu
    return _np(codes), _flat(sf, x.numel() // 32)


def _want(x, h):
    """the model on the exact y (the caller's inputs make it exact)"""
    codes, e8 = model.quantize(model.rotate(_np(x), _np(h)))
    return model.pack_e2m3(codes), e8.reshape(-1)


def _same(got, want, what):
    bad_c, bad_s = int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum())
    print(f"{what}: {bad_c} of {want[0].size} code bytes and {bad_s} of {want[1].size} scales differ from the model")
    assert bad_s == 0 and bad_c == 0, what


# ---- 1. the exact regime: zero tolerance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROTS)
def test_identity_rotation_on_gaussians_is_the_model_byte_for_byte(q, R):
    gen = torch.Generator().manual_seed(7 + R)
    for shape in SHAPES:
        for mag in (0.01, 1.0, 3000.0):
            x = (torch.randn(shape, generator=gen) * mag).to(torch.bfloat16)   # y = x: one non-zero product per sum
            _same(_run(q, x, _identity(R)), _want(x, _identity(R)), f"identity R {R} {shape} x {mag}")


@pytest.mark.parametrize("R", ROTS)
def test_non_symmetric_rotation_on_exact_inputs_is_the_model_byte_for_byte(q, R):
    h = rot.signed_permuted_hadamard(R)
    for i, shape in enumerate(SHAPES):
        x = rot.exact_input(shape, seed=100 * R + i)
        k = torch.randint(-6, 7, (*shape[:-1], 1), generator=torch.Generator().manual_seed(i))
        x = (x.float() * torch.exp2(k.float())).to(torch.bfloat16)            # a power of two per row: still exact, and the scale byte varies
        want = _want(x, h)
        _same(_run(q, x, h), want, f"R {R} {shape}")
        if i == 2:
            assert np.unique(want[1]).size >= 8 and np.unique(model.unpack_e2m3(want[0])).size >= 16


# ---- 2. the edge rows of the contract, identity rotation ---------------------------------------------------------------------------------------------------
def _midpoint_groups():
    """every midpoint between two neighbouring e2m3 magnitudes, both signs, 31 to a group whose 32nd value is +4: the group's scale byte is then 127 and the scaled
    values are the midpoints themselves -- every tie of the format"""
    vals = model.E2M3[:32]
    mids = (vals[:-1] + vals[1:]) / 2
    mids = np.concatenate([mids, -mids])
    pad = (-mids.size) % 31
    g = np.concatenate([mids, np.zeros(pad)]).reshape(-1, 31)
    return np.concatenate([g, np.full((g.shape[0], 1), 4.0)], axis=1), mids.size


@pytest.mark.parametrize("R", ROTS)
def test_edge_rows_of_the_contract(q, R):
    big = float(torch.tensor([0x7f7f], dtype=torch.uint16).view(torch.bfloat16).float())   # the largest finite bf16
    zero = np.zeros(32)
    neg0 = zero.copy(); neg0[[1, 7, 30]] = -0.0                         # a -0 INPUT: the rotation sums from +0, so y = +0 -- scale 127, codes 0
    tiny = zero.copy(); tiny[0] = 1.0; tiny[1:4] = [-2.0 ** -40, 2.0 ** -40, -2.0 ** -60]   # scaled below half the smallest step: -0 keeps its sign
    sat = zero.copy(); sat[:8] = [7.75, -7.75, 7.5, 7.25, -7.25, 7.0, 7.9375, 4.0]           # (7.5, 8) -> 7.5; 7.25 is a tie: to the even code, 7.0
    sat2 = sat * 2.0 ** -20                                              # ... the same in another scale
    den = zero.copy(); den[[3, 4, 5, 6]] = [2.0 ** -130, -2.0 ** -131, 1.5 * 2.0 ** -130, 2.0 ** -133]   # a denormal amax: E = 0, e8 = 0, scaled by 2^127
    low = zero.copy(); low[[3, 4, 5]] = [2.0 ** -125, -2.0 ** -126, 1.5 * 2.0 ** -126]      # E = 2: e8 = 0 without the clamp; E - 2 < 0 one below
    high = zero.copy(); high[[0, 9, 31]] = [big, -big, big / 2]
    mids, n_mids = _midpoint_groups()
    groups = np.concatenate([np.stack([zero, neg0, tiny, sat, sat2, den, low, high]), mids])
    groups = np.concatenate([groups, np.zeros(((-groups.shape[0]) % (R // 32), 32))])    # whole rotation blocks
    x = torch.from_numpy(groups).to(torch.bfloat16).reshape(-1, R)
    assert np.array_equal(x.double().numpy().reshape(-1, 32), groups), "every value must be a bf16 number"
    want = _want(x, _identity(R))
    codes = model.unpack_e2m3(want[0]).reshape(-1, 32)
    assert want[1][:8].tolist() == [127, 127, 125, 127, 107, 0, 0, 252] and (want[1][8:8 + mids.shape[0]] == 127).all()
    assert not codes[:2].any() and codes[2, :4].tolist() == [24, 32, 0, 32]
    assert codes[3, :8].tolist() == [31, 63, 31, 30, 62, 30, 31, 24] and codes[4, :8].tolist() == codes[3, :8].tolist()
    assert codes[5, 3:7].tolist() == [1, 32, 2, 0]                     # 2^-130 x 2^127 = 1/8; -1/16 and 3/16 are ties: to the even codes -0 and 2
    assert n_mids == 62
    tie_codes = codes[8:8 + mids.shape[0], :31].reshape(-1)[:n_mids]
    assert (tie_codes % 2 == 0).all(), "every tie goes to the even code"
    _same(_run(q, x, _identity(R)), want, f"edge rows R {R}")


# ---- 3. non-finite inputs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROTS)
def test_a_non_finite_input_poisons_its_own_rotation_block_only(q, R):
    """a NaN or an infinity makes every y of its rotation block NaN or infinite: all scale bytes of that block 255, all its codes 0, no other block touched --
    with the identity, and with a rotation that mixes the block"""
    for hname, h in (("identity", _identity(R)), ("hadamard", rot.signed_permuted_hadamard(R))):
        x = (torch.randn(33, 3 * R, generator=torch.Generator().manual_seed(90 + R)) * 2.0).to(torch.bfloat16)
        clean_c, clean_s = _run(q, x, h)
        for value, block, at in ((float("nan"), 17, 5), (float("inf"), 3 * 33 - 1, R - 1), (float("-inf"), 40, 0)):   # (a block of the first tile, the very last block, ...)
            xb = x.clone().reshape(-1, R)
            xb[block, at] = value
            c, s = _run(q, xb.reshape(x.shape), h)
            c, s, cc, cs = c.reshape(-1, R * 3 // 4), s.reshape(-1, R // 32), clean_c.reshape(-1, R * 3 // 4), clean_s.reshape(-1, R // 32)
            others = np.arange(c.shape[0]) != block
            assert np.array_equal(c[others], cc[others]) and np.array_equal(s[others], cs[others]), (hname, value, block)
            assert (s[block] == 255).all() and not c[block].any(), (hname, value, block, s[block])
    # the model agrees where y is exact: the identity
    xb = x.clone().reshape(-1, R)
    xb[17, 5], xb[40, 0] = float("nan"), float("inf")
    _same(_run(q, xb.reshape(x.shape), _identity(R)), _want(xb.reshape(x.shape), _identity(R)), f"non-finite R {R}")


# ---- 4. the gathering form -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROTS)
def test_gathering_form_is_the_plain_op_on_index_select(q, R):
    T, K = 7, 5 * R if R < 128 else 640
    gen = torch.Generator().manual_seed(50 + R)
    x = (torch.randn(T, K, generator=gen) * 5.0).to(torch.bfloat16).to(DEV)
    h = rot.general_rotation(R).to(DEV)
    xz = torch.cat([x, torch.zeros(1, K, dtype=torch.bfloat16, device=DEV)])          # row T: the zero row of a bad index
    for src in ([3], [-1], 33, 70):
        if isinstance(src, int):
            m = src
            src = torch.randint(0, T, (m,), generator=gen).tolist()                   # 7 rows for 33 / 70 indices: repeats
            for pos, bad in zip(torch.randperm(m, generator=gen)[:6].tolist(), (-1, 7, 2 ** 30, -1, 7, 2 ** 30)):
                src[pos] = bad
        M = len(src)
        idx = torch.tensor(src, dtype=torch.int32, device=DEV)
        safe = torch.tensor([i if 0 <= i < T else T for i in src], dtype=torch.int64, device=DEV)
        want_codes, want_sf = q.fusedQuantizeMxf6(xz.index_select(0, safe), h)
        got_codes, got_sf = q.fusedGatherQuantizeMxf6(x, h, idx)
        n = M * K // 32
        assert got_codes.shape == (M, K * 3 // 4) and np.array_equal(_np(got_codes), _np(want_codes)) and np.array_equal(_flat(got_sf, n), _flat(want_sf, n)), M
        for i, s in enumerate(src):
            if not 0 <= s < T:
                assert not _np(got_codes)[i].any() and (_flat(got_sf, n).reshape(M, -1)[i] == 127).all(), (i, s)
        # guard bytes around both outputs: the bytes of OUT / OUT_sf past the written range stay as they were
        out = torch.full((M + 3, K * 3 // 4), 0xff, dtype=torch.uint8, device=DEV)
        out_sf = torch.full((n + 64,), 0xff, dtype=torch.uint8, device=DEV).view(torch.float8_e8m0fnu)
        torch.ops.qutlass_amd_mxf6.fusedGatherQuantizeMxf6_(x, h, idx, out, out_sf)
        assert np.array_equal(_np(out)[:M], _np(want_codes)) and (_np(out)[M:] == 0xff).all()
        assert np.array_equal(_flat(out_sf, n), _flat(want_sf, n)) and (_np(out_sf).reshape(-1)[n:] == 0xff).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_plain_form_leaves_the_guard_bytes(q, shape):
    R = 32
    rows, K = shape
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(rows)) * 3.0).to(torch.bfloat16)
    want = _want(x, _identity(R))
    nb, n = rows * K * 3 // 4, rows * K // 32
    buf = torch.full((nb + 512,), 0xff, dtype=torch.uint8, device=DEV)
    buf_sf = torch.full((n + 128,), 0xff, dtype=torch.uint8, device=DEV)
    out, out_sf = buf[256:256 + nb].view(rows, K * 3 // 4), buf_sf[64:64 + n].view(torch.float8_e8m0fnu)
    torch.ops.qutlass_amd_mxf6.fusedQuantizeMxf6_(x.to(DEV), _identity(R).to(DEV), out, out_sf)
    torch.cuda.synchronize()
    assert (_np(buf)[:256] == 0xff).all() and (_np(buf)[256 + nb:] == 0xff).all(), "a code byte written outside the output"
    assert (_np(buf_sf)[:64] == 0xff).all() and (_np(buf_sf)[64 + n:] == 0xff).all(), "a scale byte written outside the output"
    _same((_np(out), _np(out_sf).reshape(-1)), want, f"guarded {shape}")


# ---- 5. graph capture and torch.compile ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bytes(q):
    R = 64
    gen = torch.Generator().manual_seed(3)
    h = rot.general_rotation(R).to(DEV)
    x = (torch.randn(70, 3 * R, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(-1, 71, (45,), generator=gen).to(torch.int32).to(DEV)
    calls = {"plain": lambda: q.fusedQuantizeMxf6(x, h), "gather": lambda: q.fusedGatherQuantizeMxf6(x, h, src)}
    for name, call in calls.items():
        eager = call()
        torch.cuda.synchronize()
        n = eager[0].numel() // 24
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = call()
        cap[0].view(torch.uint8).zero_()
        cap[1].view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(cap[0]), _np(eager[0])), name
        assert np.array_equal(_flat(cap[1], n), _flat(eager[1], n)), name


def test_torch_compile_fullgraph(q):
    R = 32
    x = (torch.randn(33, 256, generator=torch.Generator().manual_seed(4)) * 2.0).to(torch.bfloat16).to(DEV)
    h = _identity(R).to(DEV)
    src = torch.tensor([5, 0, 40, -1, 5], dtype=torch.int32, device=DEV)

    def both(x, h, src):
        a, asf = q.fusedQuantizeMxf6(x, h)
        g, gsf = q.fusedGatherQuantizeMxf6(x, h, src)
        return a, asf, g, gsf

    eager = both(x, h, src)
    torch._dynamo.reset()
    got = torch.compile(both, backend="inductor", fullgraph=True)(x, h, src)
    for i, n in ((0, None), (1, 33 * 8), (2, None), (3, 5 * 8)):
        e, g = _np(eager[i]).reshape(-1), _np(got[i]).reshape(-1)
        assert np.array_equal(e[:n], g[:n]), i
