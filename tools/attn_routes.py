"""Which kernels the fp32 token-attention forward runs, and what it computes, for every case of tests/attn_route_cases.py under every
split mode; with --bwd the same for the backward and tests/attn_bwd_route_cases.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/attn_routes.py [--bwd] --out routes.txt      (one MI355X)
    python tools/attn_routes.py --merge routes.txt DIR/.../*_kernel_trace.csv [--out FILE]                           (no GPU)

The first form runs every case under every split mode and writes one line per call, in call order: ``id mode status hash`` with
the sha256 of the output bytes (and of the lse bytes where the call has them; the backward: of the dqkv bytes), or the status (``ValueError`` where the ops wrapper
itself refuses) and the message of a refused call.  A one-element int16 fill is launched immediately before and after every call; the
kernel trace of the run (a run of its own, no counters) is in dispatch order, so the names between the 2 i-th and the 2 i + 1-th such
fill are the kernels of call i.  The second form cuts the trace there and prints one line per case and distinct outcome, the modes
that gave it listed behind the id:

    id@mode,mode status hash kernel; kernel

Uses the ops.token_attention* wrappers (the backward: ops.token_attention_bwd) and lime_set_split_gemm only, so it runs unchanged on any commit: two commits route and compute
alike when their merged outputs are byte-identical (profiles/attn_routes_*.txt).  Operands come from a CPU generator seeded by the
case id.  The run synchronises after each call and stops at the first fault; run it under a time limit (``timeout -k 10 300``).
"""
import argparse
import csv
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import attn_bwd_route_cases as arc_bwd  # noqa: E402
import attn_route_cases as arc  # noqa: E402

SENTINEL = 'FillFunctor<short>'        # torch's fill of an int16 tensor: nothing else in the run fills one


def short(name):
    """The kernel as the library's plan names it: no return type, namespace or parameter list."""
    return re.sub(r'\(.*$', '', name.replace('(anonymous namespace)::', '').replace('void ', ''))


def run(out_path, bwd=False):
    """bwd: the backward table.  Its results are written, so they are what is cleared before a call and hashed behind it; the forward's
    out and lse are the call's inputs there."""
    import torch
    from lime_cikm25_amd import _lib, ops
    lib = _lib.load()
    start = lib.lime_set_split_gemm(-1)
    mark = torch.empty(1, dtype=torch.int16, device='cuda')      # empty: a zeros() would be a sentinel of its own
    torch.cuda.synchronize()
    lines = []
    table, results = (arc_bwd, ('dqkv',)) if bwd else (arc, ('out', 'lse'))
    for c in table.CASES:
        fn, kw = table.build(c)
        for mode in table.MODES:
            lib.lime_set_split_gemm(mode)
            for name in results:
                if kw.get(name) is not None:
                    kw[name].zero_()
            mark.fill_(1)
            try:
                out = getattr(ops, fn)(**kw)
                status = 0 if out is not None else ops.NOT_APPLICABLE
            except _lib.LimeHipError as e:               # refused on the host before any launch
                m = re.match(r'.* failed with status (-?\d+): (.*)', str(e), re.S)
                status, out = '%s %s' % (m.group(1), ' '.join(m.group(2).split())), None
            except ValueError as e:
                status, out = 'ValueError %s' % ' '.join(str(e).split()), None
            finally:
                mark.fill_(2)
            torch.cuda.synchronize()                     # a GPU fault raises here and ends the run: nothing more is launched
            if out is not None:
                h = hashlib.sha256(out.cpu().contiguous().numpy().tobytes())
                if not bwd and kw.get('lse') is not None:
                    h.update(kw['lse'].cpu().numpy().tobytes())
                status = '0 %s' % h.hexdigest()
            line = '%s %d %s' % (c['id'], mode, status)
            print(line, flush=True)
            lines.append(line)
    lib.lime_set_split_gemm(start)
    if out_path:
        with open(out_path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def merge(calls_path, trace_path, out_path):
    with open(trace_path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: (int(r['Start_Timestamp']), int(r['Dispatch_Id'])))
    segments, current = [], None                         # kernel names between each pair of sentinels
    for r in rows:
        if SENTINEL in r['Kernel_Name']:
            if current is None:
                current = []
            else:
                segments.append(current)
                current = None
        elif current is not None:
            current.append(short(r['Kernel_Name']))
    assert current is None, 'the trace ends inside a call'
    with open(calls_path) as f:
        calls = [line.rstrip('\n').split(' ', 2) for line in f]
    assert len(calls) == len(segments), 'calls %d, sentinel pairs %d' % (len(calls), len(segments))
    outcomes = {}                                        # id -> {outcome: modes}, both in the order first seen
    for (cid, mode, status), kernels in zip(calls, segments):
        if status.startswith('0 '):
            status += ' ' + ('; '.join(kernels) if kernels else '-')
        else:
            assert not kernels, '%s@%s was refused and launched %s' % (cid, mode, kernels)
        outcomes.setdefault(cid, {}).setdefault(status, []).append(mode)
    lines = ['%s@%s %s' % (cid, ','.join(modes), status) for cid, by in outcomes.items() for status, modes in by.items()]
    print('\n'.join(lines))
    if out_path:
        with open(out_path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--bwd', action='store_true', help='the backward table (tests/attn_bwd_route_cases.py)')
    ap.add_argument('--merge', nargs=2, metavar=('CALLS', 'TRACE'))
    a = ap.parse_args()
    if a.merge:
        merge(a.merge[0], a.merge[1], a.out)
    else:
        run(a.out, a.bwd)


if __name__ == '__main__':
    main()
