"""bench.py's own contract: a plain run times the headline workload and nothing else, --dump-outputs writes what the last timed step
left (the loss and the trained parameters) as .npy files under a size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _workload():
    import bench
    torch.manual_seed(0)
    a, b = torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32)
    return bench.Workload('toy', lambda: None, 1, 'steps/s', None, lambda r: r, models=[('seg', a), ('reg', b)])


def test_dump_outputs_names_dtypes_and_values(tmp_path):
    import bench
    wl = _workload()
    n = bench.dump_outputs(str(tmp_path), 0.25, wl)
    names = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert n == len(names) == 7 and 'loss' in names and 'seg.weight' in names and 'reg.running_var' in names
    assert 'reg.num_batches_tracked' not in names                     # integer buffers are not outputs of the arithmetic
    assert np.load(tmp_path / 'loss.npy').tolist() == [0.25]
    w = np.load(tmp_path / 'seg.weight.npy')
    assert w.dtype == np.float32 and np.array_equal(w, wl.models[0][1].weight.detach().numpy())


def test_dump_outputs_samples_a_fixed_subset_past_the_budget(tmp_path, monkeypatch):
    import bench
    wl = _workload()
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 1024)
    bench.dump_outputs(str(tmp_path / 'a'), 1.0, wl)
    bench.dump_outputs(str(tmp_path / 'b'), 1.0, wl)
    sizes = 0
    for f in os.listdir(tmp_path / 'a'):
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert np.array_equal(x, y)                                     # the same sample from run to run
        sizes += x.nbytes
    assert sizes <= 1024
    w = wl.models[0][1].weight.detach().numpy().reshape(-1)
    s = np.load(tmp_path / 'a' / 'seg.weight.npy')
    assert 0 < s.size < w.size and np.isin(s, w).all()


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` at a small size: the result line carries the headline's fields for exactly K
    steps and none of --full's blocks; DIR holds the last step's loss and the UNet_light parameters, under 64 MB."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--shape', '32', '32', '32',
                          '--dump-outputs', str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{"metric"')][-1])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'volumes/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['roofline'] is None and line['extra'] is None and line['cpu_baseline'] is None
    files = os.listdir(tmp_path)
    assert 'loss.npy' in files and sum(f.startswith('seg.') for f in files) > 20
    assert sum(os.path.getsize(tmp_path / f) for f in files) < 64 << 20
    loss = np.load(tmp_path / 'loss.npy')
    assert loss.dtype == np.float32 and abs(float(loss[0]) - line['config']['final_loss']) < 1e-6
