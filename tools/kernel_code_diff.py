"""Which kernels does a source change alter?  CPU only.

    python tools/kernel_code_diff.py <tree A> <tree B>

Compiles every lime_cikm25_amd/csrc/*.hip of both trees to gfx950 assembly (device pass only, the library's flags), cuts the output
into functions and kernel descriptors (.amdhsa_kernel blocks: registers, LDS, scratch), strips comments and the numbers of
compiler-made labels, and compares by MANGLED NAME -- whichever unit a kernel lives in, so a refactor that moves kernels between
units or helpers into headers can show that it left the device code alone.  Prints the kernels that are missing, new or
different; exit status 1 when there are any.
"""
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', '-o', '-']


def functions(asm):
    """[(mangled name, normalised text)] of one unit's assembly: every function body and every kernel descriptor."""
    asm = re.sub(r'\.(LBB|Ltmp|Lfunc_end|Lfunc_begin)\d+', r'.\1', re.sub(r'[ \t]*;[^\n]*', '', asm))
    out = []
    for m in re.finditer(r'^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end:', asm, re.M | re.S):
        out.append((m.group(1), m.group(2)))
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', asm, re.M | re.S):
        out.append((m.group(1), m.group(2)))
    return out


def tree_kernels(root):
    csrc = os.path.join(root, 'lime_cikm25_amd', 'csrc')
    units = sorted(glob.glob(os.path.join(csrc, '*.hip')))
    compile_unit = lambda src: subprocess.run(['hipcc'] + FLAGS + [src], cwd=csrc, check=True, capture_output=True, text=True).stdout
    kernels = collections.defaultdict(list)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as pool:
        for asm in pool.map(compile_unit, units):
            for name, text in functions(asm):
                kernels[name].append(text)
    return {name: sorted(texts) for name, texts in kernels.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = tree_kernels(sys.argv[1]), tree_kernels(sys.argv[2])
    report = [('missing', sorted(set(a) - set(b))), ('new', sorted(set(b) - set(a))),
              ('different', sorted(n for n in set(a) & set(b) if a[n] != b[n]))]
    for what, names in report:
        for n in names:
            print('%-10s %s' % (what, n))
    print('%d functions in %s, %d in %s: %d missing, %d new, %d different' % ((len(a), sys.argv[1], len(b), sys.argv[2]) +
                                                                              tuple(len(names) for _, names in report)))
    return 1 if any(names for _, names in report) else 0


if __name__ == '__main__':
    sys.exit(main())
