"""GPU: a plain `bench.py` run (no --full) times exactly its --steps and reports only the headline figures; its inputs
are seeded, so two runs with the same arguments start from the same state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ('roofline', 'hot_path_only', 'hot_path_kernels', 'full_run', 'by_deg', 'single_chain', 'final_gather', 'cpu_baseline')


def test_bench_inputs_are_the_same_on_every_run():
    import bench
    dev = torch.device('cuda')
    a, b = (bench.build_problem(dev, 2, 0, tiny=True) for _ in range(2))
    for k in ('x', 'p', 'y'):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(u, v) for u, v in zip(a['model'].state_dict().values(), b['model'].state_dict().values()))


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    """One plain run: the line carries the headline figures of exactly --steps timed steps and none of the --full
    objects, and --dump-outputs writes the last step's x, p, xt.  (Two processes are not compared here: at this small
    --tiny-score size MIOpen's convolutions are not bit-reproducible between processes and the final clip amplifies
    their last bits; the inputs are compared directly above.)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '2',
                          '--tiny-score', '--dump-outputs', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert (line['steps'], line['warmup'], line['unit'], line['dtype'], line['higher_is_better']) == (2, 1, 'chain-steps/s', 'f32', True)
    assert line['ms_per_step'] > 0 and abs(line['value'] - 2 * 1e3 / line['ms_per_step']) <= 1e-2 * line['value']
    assert all(line[k] is None for k in EXTRAS), {k: line[k] for k in EXTRAS if line[k] is not None}
    for name in ('x', 'p', 'xt'):
        a = np.load(tmp_path / f'{name}.npy')
        assert a.dtype == np.float32 and a.shape == (2, 3, 256, 256) and np.isfinite(a).all(), name
    assert float(np.abs(np.load(tmp_path / 'xt.npy')).max()) <= 1.0                  # the clipped decode
