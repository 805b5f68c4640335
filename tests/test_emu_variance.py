"""CPU tier: the predictive variance of every route against its extended-precision value, on the emulated build of the
unmodified HIP sources (tests/emu).  N = 330, d = 4 (Np = 384: ragged last block), two outputs, sn = 1e-2 and 0.1.  The checks
live in variance_cases.py; the GPU tier runs the same ones at N = 330 and N = 1024, d = 6.  A route is given every probe, or --
where an emulated call is slow -- every second or fourth window of them (the truth and numpy's error scale are those of all 256).
Not here: the prediction behind a fit's tail, which does not exist at this size (a one-output fit at Np = 384 is a single worker
launch and returns with its tail done); the GPU tier gates it at N = 1024."""
import os
import subprocess

import pytest

import variance_cases as vc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [dict(N=330, d=4, sn=1e-2), dict(N=330, d=4, sn=0.1)]
IDS = ['sn1e-2', 'sn0.1']


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_yardstick_certifies_itself(size):
    vc.model(**size)


@pytest.mark.parametrize('B', [1, 5, 32, 33, 64, 65])
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_predict_mean_var_batch_sizes(emu, size, B):
    vc.check_batch_size(emu, B, stride={1: 4, 5: 2}.get(B, 1), **size)      # (an emulated call is 50 ms: 64 of the 256 probes at B = 1)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_large_batch_tile_gemm_and_persistent(emu, size):
    vc.check_large_batch(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_probes_span_chunks(emu, size):
    vc.check_chunked(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_fused_fit_predict(emu, size):
    vc.check_fused_fit_predict(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_predict_me_and_ta_diagonals(emu, size):
    vc.check_moment_methods(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_predict_sens_var_and_dvar(emu, size):
    vc.check_sens(emu, sizes=(33,), **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_covar(emu, size):
    vc.check_covar(emu, **size)


@pytest.mark.parametrize('N0', [320, 300, 250])        # the strip update (10 new rows), and two refits
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_after_append(emu, size, N0):
    vc.check_after_append(emu, N0, stride=4, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_after_set_factors(emu, size):
    vc.check_after_set_factors(emu, stride=2, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_rollout_first_step(emu, size):
    vc.check_rollouts(emu, stride=4, **size)
