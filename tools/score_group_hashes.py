"""What Model.score_pool / recommend / score_lists / recommend_lists compute, bit for bit, on the tiny models of tests/test_recommend_gpu.py
and tests/test_lists_gpu.py: per case name one line per call, ``file case call sha256 ...`` with the sha256 of every returned tensor's bytes.
Public methods and the tests' ``build`` only, so it runs on any commit that has them: two commits compute alike when their outputs are
byte-identical (profiles/score_groups_*.txt) and launch alike when the per-kernel call counts of a ``rocprofv3 --kernel-trace --stats``
run of it (a run of its own, no counters) agree.  It synchronises after each call and stops at the first fault; run it under a time limit."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch  # noqa: E402
import test_lists_gpu as lists  # noqa: E402
import test_recommend_gpu as pool  # noqa: E402

for mod, score, rec, passes, ks in ((pool, 'score_pool', 'recommend', 40, (5, pool.C)),
                                    (lists, 'score_lists', 'recommend_lists', 1, (4, lists.LENS[0]))):
    for case in mod.CASES:
        model, args, _, n_src = mod.build(case)[:4]
        calls = [(score, dict(kw, exclude_history=ex)) for kw in ({}, {'pairs_per_pass': passes}) for ex in (False, True)]
        calls += [(rec, dict(k=k, exclude_history=ex)) for k in ks for ex in (False, True)]
        for fn, kw in calls:
            out = getattr(model, fn)(**args, n_src=n_src, **kw)
            torch.cuda.synchronize()                     # a GPU fault raises here and ends the run: nothing more is launched
            hashes = [hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest() for t in (out if isinstance(out, tuple) else (out,))]
            print(mod.__name__, case, fn, *['%s=%s' % kv for kv in sorted(kw.items())], *hashes, flush=True)
