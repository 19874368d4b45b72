#!/usr/bin/env python3
"""Do two builds of one translation unit of csrc/capi.hip hold the same kernels, instruction for instruction?  Takes the device assembly of the unit from two
source trees (the command below, once per tree) and compares every kernel that both hold: the instruction stream with block labels renumbered away, and the
kernel descriptor's VGPR / SGPR / LDS / scratch figures.  A change to a shared parameter struct moves the hidden kernel arguments behind it, so a kernel that
differs ONLY in the constant of an s_load from / s_add to the kernarg pointer is reported as "same up to kernarg offsets", not as different.  Kernels only one
side has are listed with their resources.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden [-mllvm -amdgpu-mfma-vgpr-form] -DQAMD_TU=5 --cuda-device-only -S \\
          qutlass_amd/csrc/capi.hip -o new.s            # (the per-unit flags of qutlass_amd/build.py TU_FLAGS)
    python tools/isa_diff.py old.s new.s [--show]       # --show: print the differing lines of every kernel reported as different

Exit status 1 if a kernel both sides hold differs in more than kernarg offsets."""
from __future__ import annotations

import re
import shutil
import subprocess
import sys


def kernels(path):
    """name -> (instructions, descriptor figures) of every kernel of one assembly file"""
    txt = open(path).read()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        fig = lambda k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)).group(1))
        meta[m.group(1)] = dict(vgpr=fig("next_free_vgpr"), sgpr=fig("next_free_sgpr"), lds=fig("group_segment_fixed_size"), scratch=fig("private_segment_fixed_size"))
    code, cur, name = {}, None, None
    for line in txt.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None and m.group(1) in meta:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            code[name], cur = cur, None
            continue
        t = line.split(";")[0].strip()
        if re.match(r"^\.LBB\d+_\d+:$", t):
            cur.append("LABEL")
        elif t and not t.startswith("."):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return {n: (code[n], meta[n]) for n in code}


def no_kernarg_offsets(line):
    if re.match(r"s_load_\w+ \S+ s\[\d+:\d+\], 0x[0-9a-f]+$", line) or re.match(r"s_add_u32 s\d+, s\d+, 0x[0-9a-f]+$", line):
        return re.sub(r"0x[0-9a-f]+$", "K", line)
    return line


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = "--show" in sys.argv
    a, b = kernels(paths[0]), kernels(paths[1])
    names = sorted(set(a) | set(b))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    dem = dict(zip(names, subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines())) if filt else {n: n for n in names}
    same = offs = 0
    bad = []
    for n in names:
        if n not in a or n not in b:
            print("only in", paths[0] if n in a else paths[1], ":", dem[n], (a.get(n) or b.get(n))[1])
            continue
        (ca, ma), (cb, mb) = a[n], b[n]
        if ma == mb and ca == cb:
            same += 1
        elif ma == mb and [no_kernarg_offsets(x) for x in ca] == [no_kernarg_offsets(x) for x in cb]:
            offs += 1
        else:
            bad.append(n)
            print("DIFFERENT:", dem[n], len(ca), "/", len(cb), "instructions", ma, mb)
            if show:
                for x, y in zip(ca, cb):
                    if x != y:
                        print("    ", x, " | ", y)
    print(f"kernels in both: {same + offs + len(bad)}; same instructions: {same}; same up to kernarg offsets: {offs}; different: {len(bad)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
