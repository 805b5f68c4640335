"""`python bench.py --gpus N` must start its N ranks itself (the driver calls it without torchrun), print ONE line with
n_gpus = N, and carry the restart shard -- the one part of the path that shards -- in it.  CPU tier: the ranks talk over
gloo and compute on the emulated library (test infrastructure, tests/emu; GPMPC_BENCH_LIB exists for this test only)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..'))


def run_bench(*flags, env=None, timeout=900):
    e = dict(os.environ, GPMPC_BENCH_LIB=os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(flags), capture_output=True, text=True,
                       cwd=ROOT, timeout=timeout, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_gpus_2_launches_two_ranks_and_reports_the_restart_shard():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    j = run_bench('--gpus', '2', '--N', '128', '--B', '64', '--steps', '2', '--warmup', '1', '--restarts', '4',
                  '--full', '--no-cpu-baseline')
    assert j['n_gpus'] == 2 and j['steps'] == 2 and j['scaling'] == 'weak'
    assert j['config']['N'] == 128 and j['value'] > 0
    rs = j['restart_shard']
    assert rs['scaling'] == 'strong' and rs['unit'] == 'restarts/s' and rs['value'] > 0
    assert rs['config']['restarts'] == 4 and rs['restarts_this_rank'] == 2      # rank 0 ran restarts 0 and 2
    assert rs['finite_restarts'] == 4                                             # ... and received 1 and 3
    assert rs['rccl_ranks'] == 0 and 'host merge' in rs['exchange']              # no RCCL on a CPU box
    # the record validates itself: the sharded table equals the one-rank search of the same seeds bit for bit
    sc = rs['shard_check']
    assert sc['bitwise_equal_to_world1'] is True and sc['table_sha16'] == sc['world1_table_sha16']
    assert sc['theta_star_sha16'] == sc['world1_theta_star_sha16']


@pytest.mark.timeout(1200)
def test_config_c4_under_an_external_launcher_env():
    """The torch.distributed.run form: the ranks come from the environment, --gpus only names them."""
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    e = dict(os.environ, GPMPC_BENCH_LIB=os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'), WORLD_SIZE='2',
             MASTER_ADDR='127.0.0.1', MASTER_PORT='29533')
    procs = []
    for r in range(2):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--config', 'C4', '--N', '96',
                                       '--restarts', '4', '--steps', '1', '--warmup', '0'],
                                      env=dict(e, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, cwd=ROOT))
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs[0][1][-2000:] + outs[1][1][-2000:]
    assert outs[1][0].strip() == ''                                              # only rank 0 prints
    j = json.loads(outs[0][0].strip())
    assert j['n_gpus'] == 2 and j['scaling'] == 'strong' and j['finite_restarts'] == 4


@pytest.mark.timeout(1200)
def test_plain_run_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    """A plain run is the headline alone (the rest is --full's), times exactly --steps steps after --warmup, and
    --dump-outputs writes the last timed step's mean / variance: the same bits from run to run and with --full."""
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    dumps = []
    for k, (steps, warmup) in enumerate(((3, 1), (1, 0))):
        j = run_bench('--N', '128', '--B', '64', '--steps', str(steps), '--warmup', str(warmup), '--dump-outputs', str(tmp_path / str(k)))
        assert j['n_gpus'] == 1 and j['steps'] == steps and j['warmup'] == warmup
        assert j['unit'] == 'predictions/s' and j['higher_is_better'] is True and j['dtype'] == 'f64'
        assert j['ms_per_step'] > 0 and abs(j['value'] - 64 * 1e3 / j['ms_per_step']) <= 1e-6 * j['value']
        assert j['chained_factorisations'] + j['single_queue_factorisations'] == steps + warmup     # one fit per step
        assert not {'roofline', 'cholesky', 'phases_ms_per_step', 'ms_per_step_other_api', 'cpu_baseline', 'secondary'} & set(j)
        dumps.append({n: np.load(tmp_path / str(k) / f'{n}.npy') for n in ('mean', 'var')})
    j = run_bench('--N', '128', '--B', '64', '--steps', '2', '--warmup', '1', '--full', '--no-secondary',
                  '--dump-outputs', str(tmp_path / 'full'))
    assert {'roofline', 'cholesky', 'phases_ms_per_step', 'ms_per_step_other_api', 'cpu_baseline', 'parity_vs_oracle'} <= set(j)
    assert j['parity_vs_oracle']['mean_rel_to_max'] <= 1e-10
    dumps.append({n: np.load(tmp_path / 'full' / f'{n}.npy') for n in ('mean', 'var')})
    for n in ('mean', 'var'):
        assert dumps[0][n].shape == (64, 1) and dumps[0][n].dtype == np.float64 and np.all(np.isfinite(dumps[0][n]))
        assert all(np.array_equal(dumps[0][n], d[n]) for d in dumps[1:])


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 8 * 1000)
    a, b = np.arange(2000.0).reshape(1000, 2), np.arange(1000, dtype=np.float32)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), {'a': a, 'b': b})
    sa, sb = np.load(tmp_path / '0' / 'a.npy'), np.load(tmp_path / '0' / 'b.npy')
    assert sa.dtype == sb.dtype == np.float64 and sa.nbytes + sb.nbytes <= 8 * 1000 and len(sa) == len(sb) > 0
    assert np.array_equal(sa[:, 0] / 2, sb) and np.all(np.diff(sb) > 0)              # the same rows of both, in order
    assert np.array_equal(sa, np.load(tmp_path / '1' / 'a.npy')) and np.array_equal(sb, np.load(tmp_path / '1' / 'b.npy'))
