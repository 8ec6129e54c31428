#!/usr/bin/env python3
"""Compare the gfx950 machine code of two source trees, kernel by kernel.

    tools/kernel_isa_diff.py <tree A> <tree B>

Each tree's kernel translation units (gaussianrenderer_amd/csrc/*.hip) are compiled to device
assembly with that tree's Makefile HIPFLAGS (hipcc --cuda-device-only -S, at most 8 at a time)
and split per .amdhsa_kernel name; labels, comments and debug / ident lines are normalised
away.  Per kernel: are the instruction text and the VGPR / SGPR / LDS / scratch figures of the
kernel descriptor equal; and which kernels only one side has.  A kernel found in several
translation units of one tree differs.  Exit status 0 iff everything is equal.
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
           "private_segment_fixed_size")


def make_var(tree, name):
    return subprocess.run(["make", "-s", "--eval", f"isa-diff-var: ; @echo $({name})", "isa-diff-var"], cwd=tree,
                          check=True, capture_output=True, text=True).stdout.split()


def normalise(line):
    line = line.split(";")[0].strip()
    if not line or re.match(r"\.(loc|file|ident|cfi_\w+|p2align|section|text)\b", line):
        return None
    return re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def kernels(tree):
    """name -> [(instruction lines, figures)], one entry per translation unit that holds the kernel."""
    hipcc, flags = make_var(tree, "HIPCC")[0], make_var(tree, "HIPFLAGS")
    srcs = sorted(glob.glob(os.path.join(tree, "gaussianrenderer_amd", "csrc", "*.hip")))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        def one(src):
            out = os.path.join(tmp, os.path.basename(src) + ".s")
            subprocess.run([hipcc, *flags, "-x", "hip", "--cuda-device-only", "-S", os.path.relpath(src, tree),
                            "-o", out], cwd=tree, check=True)
            return open(out).read()
        found = {}
        for asm in pool.map(one, srcs):
            lines = asm.splitlines()
            for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
                name, desc = m.group(1), dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
                start = next(i for i, l in enumerate(lines) if l.startswith(name + ":")) + 1
                end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
                body = [n for n in map(normalise, lines[start:end]) if n is not None]
                found.setdefault(name, []).append((body, tuple(desc.get(f, "-") for f in FIGURES)))
    return found


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    both = sorted(set(ka) & set(kb))
    for name in sorted(set(ka) ^ set(kb)):
        print(f"ONLY IN {'A' if name in ka else 'B'}  {name}")
    equal = 0
    for name in both:
        once = len(ka[name]) == 1 and len(kb[name]) == 1
        (ia, fa), (ib, fb) = ka[name][0], kb[name][0]
        equal += once and ia == ib and fa == fb
        print(f"{'equal  ' if once and ia == ib and fa == fb else 'DIFFERS'}  {name}: "
              + (f"instructions {'equal' if ia == ib else 'differ'} ({len(ia)} / {len(ib)} lines), figures "
                 f"{'equal' if fa == fb else f'{fa} / {fb}'}" if once else
                 f"in {len(ka[name])} / {len(kb[name])} translation units"))
    one_sided = len(set(ka) ^ set(kb))
    print(f"kernels: A {len(ka)}, B {len(kb)}, on both sides {len(both)}; equal instructions and figures "
          f"({', '.join(FIGURES)}): {equal}; differing: {len(both) - equal}; on one side only: {one_sided}")
    return 0 if equal == len(both) and not one_sided else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]) if len(sys.argv) == 3 else __doc__)
