"""GPU: a plain `bench.py` run -- set-up, warm-up, ONE block of --steps timed steps, the headline line -- and
--dump-outputs, which writes what the timed step computed in its last step; two runs with the same arguments
compute the same arrays (seeded inputs, deterministic mode)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'TUCH_BENCH_BACKEND'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    dirs = [str(tmp_path / 'a'), str(tmp_path / 'b')]
    for d in dirs:
        line = _run('--steps', '4', '--warmup', '2', '--dump-outputs', d)
        assert line['steps'] == 4 and line['warmup'] == 2 and line['n_gpus'] == 1
        assert line['unit'] == 'body-fit iterations/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
        assert line['ms_per_step'] > 0 and abs(line['value'] - 64e3 / line['ms_per_step']) <= 1e-3 * line['value']
        assert line['config']['bodies'] == 64.0 and np.isfinite(line['config']['loss_sum'])
        # what only --full measures stays out of a plain run
        for key in ('repeat_ms_per_step', 'selfcheck', 'kernels_per_step', 'roofline', 'rccl_smoke', 'cpu_baseline',
                    'shard_sweep'):
            assert key not in line, key
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {'loss_sum.npy', 'bodies.npy', 'body_pose.npy', 'global_orient.npy'} <= set(names), names
    assert sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names) <= 64 * 2 ** 20
    got = {n: np.load(os.path.join(dirs[0], n)) for n in names}
    assert got['body_pose.npy'].shape == (64, 69) and got['global_orient.npy'].shape == (64, 3)
    assert float(got['bodies.npy']) == 64.0 and np.isfinite(got['loss_sum.npy']).all()
    for n in names:
        assert got[n].dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(got[n], np.load(os.path.join(dirs[1], n)), err_msg=n)
