"""Differential of the rotate + quantize family's C entries between two builds of libqutlass_amd.so, on the CPU (no GPU: every call ends before any HIP call).

    python tools/quantize_family_diff.py dump /path/to/libqutlass_amd.so a.txt      # once per library, each in its own process (both export the same C names)
    python tools/quantize_family_diff.py dump /other/libqutlass_amd.so b.txt
    python tools/quantize_family_diff.py compare a.txt b.txt

The grid is the one of tests/test_quantize_family_cpu.py (rotation x method x blocked x mask x broken pointers) over a few hundred shapes per entry: the cross of the
boundary values below, with non-multiples of the row unit, negative and >= 2^31 sizes.  A call whose checks all pass would launch and is left out.  One line per
call: its arguments, the return code and the message."""
import ctypes
import importlib.util
import itertools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("family", os.path.join(ROOT, "tests", "test_quantize_family_cpu.py"))
family = importlib.util.module_from_spec(spec)
spec.loader.exec_module(family)

from qutlass_amd import _lib   # noqa: E402  (the argument types of the C ABI)

P31 = 1 << 31
VALUES = (-1, 0, 1, 16, 31, 32, 48, 64, 96, 100, 128, 160, 256, 1000, 4096, 1 << 15, 1 << 20, (1 << 21) - 1, 1 << 21, 1 << 29, P31 - 128, P31 - 1, P31, P31 + 1, 1 << 33)
X = family.X
POINTERS = [dict(), dict(x=None), dict(h=None), dict(sf=None), dict(gs=None), dict(src_row=None), dict(h=X + 2), dict(x=X + 4), dict(src_row=X + 2)]


def shapes(kind):
    if kind == "flat":
        return [dict(numel=n) for n in sorted(set(VALUES) | {a * b for a, b in itertools.product(VALUES, VALUES) if 0 < a * b < 1 << 40})]
    if kind in ("blocked", "gated"):
        return [dict(rows=r, k=k) for r, k in itertools.product(VALUES, VALUES)]
    rng = random.Random(0)
    return [dict(t=rng.choice(VALUES), k=rng.choice(VALUES), m=rng.choice(VALUES)) for _ in range(600)]


def dump(lib_path, out_path):
    lib = ctypes.CDLL(lib_path)
    for name in list(family.ENTRIES) + ["qutlass_amd_last_error"]:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SYMBOLS[name]
    n = 0
    with open(out_path, "w") as f:
        for entry, (kind, _, args) in family.ENTRIES.items():
            for a in family.cases(entry, shapes(kind), POINTERS):
                if family.expect(entry, a) == family.LAUNCH:
                    continue
                rc, msg = family.call(lib, entry, a)
                f.write(f"{entry} {[a[k] for k in args]} -> {rc} {msg}\n")
                n += 1
    print(n, "calls written to", out_path)


def compare(a_path, b_path):
    a, b = open(a_path).read().splitlines(), open(b_path).read().splitlines()
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    print(f"{len(a)} and {len(b)} tuples, {len(diff)} differ")
    for x, y in diff[:20]:
        print(" ", x, "\n ", y)
    return 1 if diff or len(a) != len(b) else 0


if __name__ == "__main__":
    sys.exit(dump(*sys.argv[2:]) if sys.argv[1] == "dump" else compare(*sys.argv[2:]))
