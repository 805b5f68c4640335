"""CPU tier: the predictive mean, its Jacobian, its Hessian and the off-diagonal 'TA' covariance of every route against their
extended-precision values on the device's own alpha, on the emulated build of the unmodified HIP sources (tests/emu).  The
checks live in first_order_cases.py (docs/first_order_gates.md: cases, routes, bars); the GPU tier runs the same ones at
d = 6 and N up to 2050.  A route is given every probe, or -- where an emulated call is slow -- every 2nd, 4th, ... window of them
(the truth and numpy's error scale are those of all 256).
Not here: the prediction behind a fit's tail (a one-output fit at Np = 384 is a single worker launch and returns with its tail
done: no early return at this size, so only the fused call is run, which then takes the plain route inside), and the shape at
which the last training-point chunk is non-empty (Np = 2048 on the GPU): a finish kernel that stops one chunk short cannot be
seen at Np = 576, where chunks 3-7 are empty."""
import os
import subprocess

import pytest

import first_order_cases as fc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [dict(N=330, d=4, sn=1e-2), dict(N=330, d=4, sn=0.1)]
IDS = ['sn1e-2', 'sn0.1']
CHUNKED = dict(N=520, d=4, sn=1e-2)     # Np = 576 >= the emulated threshold 512: chunks 0-1 full, chunk 2 with 64 rows, 3-7 empty


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('B', [1, 5, 8, 9, 32, 33, 64, 65])
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_mean_batch_sizes(emu, size, B):
    fc.check_mean_batch(emu, B, stride={1: 8, 5: 4, 8: 2, 9: 2}.get(B, 1), **size)


@pytest.mark.parametrize('B', [3, 33, 65])
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_mean_jac_and_ta(emu, size, B):
    fc.check_jac_batch(emu, B, stride={3: 8}.get(B, 1), **size)


@pytest.mark.parametrize('B', [1, 30, 64])
def test_emu_training_point_chunks(emu, B):
    fc.check_chunk_route(emu, B, stride={1: 16, 30: 2}.get(B, 1), **CHUNKED)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_fused_fit_predict(emu, size):
    fc.check_fused_fit_predict(emu, repeat=1, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_mean_from_persistent_variance_product(emu, size):
    fc.check_fused_mean(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_predict_sens_hessian(emu, size):
    fc.check_sens(emu, 33, **size)


@pytest.mark.parametrize('d', [1, 16])
def test_emu_first_and_last_input_dimension(emu, d):
    fc.check_edges(emu, B=9, stride=4, **fc.EDGE_SIZES[d])


@pytest.mark.parametrize('kind', ['const', 'linear', 'polynomial'])
def test_emu_prior_mean_functions(emu, kind):
    fc.check_edges(emu, B=33, **fc.PRIOR_SIZES[kind])


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_rollout_first_step(emu, size):
    fc.check_rollouts(emu, stride=16, **size)
