"""Which kernel lime_linear_f32 runs, and what it computes, for every case of tests/linear_route_cases.py under every split mode.

    python tools/linear_routes.py [--out FILE]

Every case runs under every split mode; one line per case and distinct outcome, the modes that gave it listed behind the id:
``id@mode,mode status kernel sha256-of-the-output-bytes``; a refused call prints its status (or ``ValueError`` where ops.linear itself
refuses), ``-`` for kernel and hash, and the message.  Uses ops.linear, lime_set_split_gemm and
lime_last_linear_kernel() only, so it runs unchanged on any commit: two commits route and compute alike when their outputs are
byte-identical (profiles/linear_routes_*.txt).  Operands come from a CPU generator seeded by the case id.  One process, one MI355X;
run it under a time limit (``timeout -k 10 300 python tools/linear_routes.py``).
"""
import argparse
import hashlib
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import linear_route_cases as lrc  # noqa: E402
from lime_cikm25_amd import _lib, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    a = ap.parse_args()
    lib = _lib.load()
    start = lib.lime_set_split_gemm(-1)
    lines = []
    for c in lrc.CASES:
        kw = lrc.build(c)
        outcomes = {}                                    # outcome -> the modes that gave it, in the order first seen
        for mode in lrc.MODES:
            lib.lime_set_split_gemm(mode)
            kw['out'].zero_()
            if 'ln_rstd' in kw:
                kw['ln_rstd'].zero_()
            try:
                out = ops.linear(**kw)
                torch.cuda.synchronize()             # a GPU fault raises here and ends the run: nothing more is launched
                h = hashlib.sha256(out.cpu().contiguous().numpy().tobytes())
                if 'ln_rstd' in kw:
                    h.update(kw['ln_rstd'].cpu().numpy().tobytes())
                outcome = '0 %s %s' % (lib.lime_last_linear_kernel().decode(), h.hexdigest())
            except _lib.LimeHipError as e:               # refused on the host before any launch
                m = re.match(r'.* failed with status (-?\d+): (.*)', str(e), re.S)
                outcome = '%s - - %s' % (m.group(1), m.group(2))
            except ValueError as e:
                outcome = 'ValueError - - %s' % e
            outcomes.setdefault(outcome, []).append(mode)
        for outcome, modes in outcomes.items():
            line = '%s@%s %s' % (c['id'], ','.join(str(m) for m in modes), outcome)
            print(line, flush=True)
            lines.append(line)
    lib.lime_set_split_gemm(start)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
