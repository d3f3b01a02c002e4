"""bench.py's plain run: one JSON line with the headline fields over exactly --steps timed steps, none of what --full adds,
and with --dump-outputs the last timed step's outputs as float32 .npy files, equal between two runs with the same arguments.

These tests start child processes, which must not happen from a process that has initialised the GPU: conftest.py moves them to
the FRONT of the session and this module never touches the device itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(workload, out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', workload, '--steps', '3',
                        '--warmup', '2', '--dump-outputs', str(out_dir)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize('workload, names', [('cfg1', ('logits',)), ('train2b', ('loss', 'params'))])
def test_plain_run_dumps_reproducible_outputs(tmp_path, workload, names):
    runs = [_bench(workload, tmp_path / str(i)) for i in range(2)]
    for out in runs:
        assert out['steps'] == 3 and out['ms_per_step'] > 0 and out['value'] > 0 and out['higher_is_better'] is True
        assert out['unit'] == 'impressions/s' and out['dtype'] == 'f32'
        assert not {'also', 'sustained', 'cpu_baseline', 'roofline', 'dense'} & set(out)
    assert sorted(os.listdir(tmp_path / '0')) == sorted(n + '.npy' for n in names)
    total = 0
    for n in names:
        a, b = (np.load(tmp_path / str(i) / (n + '.npy')) for i in range(2))
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all()
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    if workload == 'cfg1':
        assert np.load(tmp_path / '0' / 'logits.npy').shape == (8, 2)
