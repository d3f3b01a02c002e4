"""Host time of ``Model._kept_key()``, the check in front of every graph replay ("Kept across forwards: the protocol"),
for the cfg2a (LIME-MHSA) and cfg2b (LIME-CROWN) models of bench.py on the GPU.

    python tools/bench_kept_key.py

One forward first, so that what the encoders keep exists; then 5 repeats of 20000 calls under ``time.perf_counter``.  One line per
model: the 5 per-call times in microseconds.  Nothing changes between the calls, so every one of them takes the path of nearly every
forward: sources fetched, state built, one comparison."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import bench  # noqa: E402

REPEATS, CALLS = 5, 20000


def main():
    import torch
    for name in ('cfg2a', 'cfg2b'):
        run = bench.Run(name, 0, 1)
        run.step()
        torch.cuda.synchronize()
        key = run.model._kept_key
        first = key()
        per_call = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                key()
            per_call.append((time.perf_counter() - t0) / CALLS * 1e6)
        assert key() == first
        print('%s _kept_key us per call: %s   key %r' % (name, ' '.join('%.3f' % t for t in per_call), first), flush=True)


if __name__ == '__main__':
    main()
