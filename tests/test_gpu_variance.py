"""GPU tier (-m gpu): the predictive variance of every route against its extended-precision value on a real MI355X.  N = 330
(chain + flagged GEMMs) and N = 1024 (two-level factorisation), d = 6, two outputs, sn = 1e-2 and 0.1; the yardstick of a model
is evaluated once (host, seconds) and shared by every route.  The checks live in variance_cases.py; the emulator tier runs the
same ones at N = 330, d = 4."""
import pytest

import variance_cases as vc

pytestmark = pytest.mark.gpu

SIZES = [dict(N=330, d=6, sn=1e-2), dict(N=330, d=6, sn=0.1), dict(N=1024, d=6, sn=1e-2), dict(N=1024, d=6, sn=0.1)]
IDS = ['N330sn1e-2', 'N330sn0.1', 'N1024sn1e-2', 'N1024sn0.1']
SMALL, SMALL_IDS = SIZES[:2], IDS[:2]


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_yardstick_certifies_itself(size):
    vc.model(**size)


@pytest.mark.parametrize('B', [1, 5, 32, 33, 64, 65])
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_predict_mean_var_batch_sizes(lib, size, B):
    vc.check_batch_size(lib, B, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_large_batch_tile_gemm_and_persistent(lib, size):
    vc.check_large_batch(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_probes_span_chunks(lib, size):
    vc.check_chunked(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_fused_fit_predict(lib, size):
    vc.check_fused_fit_predict(lib, **size)


@pytest.mark.parametrize('size', SIZES[2:], ids=IDS[2:])
def test_prediction_behind_the_fits_tail(lib, size):
    # (N = 1024 only: at Np = 384 the one-output fit is a single worker launch and does not return before its tail)
    vc.check_behind_tail(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_predict_me_and_ta_diagonals(lib, size):
    vc.check_moment_methods(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_predict_sens_var_and_dvar(lib, size):
    vc.check_sens(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_covar(lib, size):
    vc.check_covar(lib, **size)


@pytest.mark.parametrize('N0', [320, 300, 250])        # the strip update (10 new rows), and two refits
@pytest.mark.parametrize('size', SMALL, ids=SMALL_IDS)
def test_after_append(lib, size, N0):
    vc.check_after_append(lib, N0, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_after_set_factors(lib, size):
    vc.check_after_set_factors(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_rollout_first_step(lib, size):
    vc.check_rollouts(lib, **size)
