"""Write footprint of every MX GEMM kernel form (tests/_mx_cases.py) at ragged shapes, through the lab library's C entries: D is rows [G, G + M) of a bf16 buffer
pre-filled with a NaN payload no kernel produces (G = 256 rows, one tile of the largest form) -- both guard bands keep it in every element and every element of D is
written; the _ws entries and the NN op get their queried workspace plus a 1 MiB sentinel tail, which stays untouched; the grouped ops run with offs[-1] == M."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402,F401
import _benchlib as lab  # noqa: E402,F401
import _mx_cases as mc  # noqa: E402


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


@pytest.mark.parametrize("c", mc.CASES, ids=lambda c: c.id)
def test_nothing_outside_d_and_the_stated_workspace_is_written(q, c):
    d = mc.dataset(c, "extremes")
    r = mc.run(c, d)
    mc.assert_footprint(r)
    if any(k == "splitk_force" for k, _ in c.opts) or c.op == "nn":
        assert r.ws_bytes > 0
    mc.assert_equals_reference(r.out, d.ref)
