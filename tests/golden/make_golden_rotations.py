#!/usr/bin/env python3
"""Golden vectors that pin which way round the quantizers apply a rotation that is NOT its own transpose.

make_golden.py feeds the reference's Python test oracles the Sylvester matrix almost everywhere (one random h at R = 32 for MX, none for NV), and that matrix equals
its transpose: an oracle computing x @ h.T would reproduce those fixtures.  This script adds the missing cases to a fixture of its own, quantize_rot.npz (the other
fixtures and make_golden.py's random stream stay as they are):

  * NV `_forward_quantize_ref` (tests/nvfp4_test.py:132-170) at R = 16, 32, 64, 128;
  * MX `_forward_quantize_ref` (tests/mxfp4_test.py:135-184) at R = 64 and 128, quest and abs_max;
  * each once with the signed, row-permuted Hadamard matrix of tests/_rotations.py and once with a general 0.2 * randn(R, R); x is randn(4, 512) * 25.

The reference's oracles are imported (make_golden.load_reference), not copied.  Run in the build container: python tests/golden/make_golden_rotations.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (load_reference(), bits16(), u8())
import _rotations as rot  # noqa: E402  (tests/_rotations.py)


def main():
    _utils, mx, nv, _f8 = mg.load_reference()
    torch.manual_seed(23)
    d, case = {}, 0
    for fmt, R, quest in [("nv", r, False) for r in (16, 32, 64, 128)] + [("mx", r, qs) for r in (64, 128) for qs in (True, False)]:
        for kind, h in (("hadamard", rot.signed_permuted_hadamard(R, seed=case)), ("general", rot.general_rotation(R, seed=case))):
            assert not torch.equal(h, h.T.contiguous())
            x = torch.randn(4, 512, dtype=torch.bfloat16) * 25.0
            if fmt == "nv":
                _, _, (e2m1, sf, _) = nv._forward_quantize_ref(x, h, R)
            else:
                _, _, (e2m1, sf, mask) = mx._forward_quantize_ref(x, h, R, quest=quest)
                d[f"mask{case}"] = mg.u8(mask)
            d[f"x{case}"], d[f"h{case}"] = mg.bits16(x), mg.bits16(h)
            d[f"e2m1_{case}"], d[f"sf{case}"] = mg.u8(e2m1), mg.u8(sf)
            d[f"meta{case}"] = np.array([int(fmt == "nv"), R, int(quest), int(kind == "general")])
            case += 1
    d["ncases"] = np.array(case)
    out = os.path.join(HERE, "quantize_rot.npz")
    np.savez_compressed(out, **d)
    print("wrote quantize_rot.npz:", case, "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
