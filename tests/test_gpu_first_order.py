"""GPU tier (-m gpu): the predictive mean, its Jacobian, its Hessian and the off-diagonal 'TA' covariance of every route against
their extended-precision values on the device's own alpha, on a real MI355X.  N = 330 and 1024, d = 6, two outputs, sn = 1e-2 and
0.1; N = 2048 and 2050 for the training-point chunk route; d = 1, 9, 16 and the prior mean functions at small N.  The yardstick of
a model and alpha is evaluated once (host, about a second at N = 2050) and shared by every route.  The checks live in
first_order_cases.py (docs/first_order_gates.md: cases, routes, bars); the emulator tier runs the same ones at d = 4."""
import pytest

import first_order_cases as fc

pytestmark = pytest.mark.gpu

SIZES = [dict(N=330, d=6, sn=1e-2), dict(N=330, d=6, sn=0.1), dict(N=1024, d=6, sn=1e-2), dict(N=1024, d=6, sn=0.1)]
IDS = ['N330sn1e-2', 'N330sn0.1', 'N1024sn1e-2', 'N1024sn0.1']
SMALL, SMALL_IDS = SIZES[:2], IDS[:2]
# Np = 2048: eight one-pass chunks, the last one live; N = 2050, Np = 2112: chunk 4 holds 64 rows, two of them live, 5-7 are empty
CHUNKED, CHUNKED_IDS = [dict(N=2048, d=6, sn=1e-2), dict(N=2050, d=6, sn=1e-2)], ['N2048', 'N2050']


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('B', [1, 5, 8, 9, 32, 33, 64, 65])
@pytest.mark.parametrize('size', SMALL, ids=SMALL_IDS)
def test_mean_batch_sizes(lib, size, B):
    fc.check_mean_batch(lib, B, **size)


@pytest.mark.parametrize('B', [1, 3, 4, 5, 33, 65, 256])
@pytest.mark.parametrize('size', SMALL, ids=SMALL_IDS)
def test_mean_jac_and_ta(lib, size, B):
    fc.check_jac_batch(lib, B, **size)


@pytest.mark.parametrize('B', [1, 30, 64])
@pytest.mark.parametrize('size', CHUNKED, ids=CHUNKED_IDS)
def test_training_point_chunks(lib, size, B):
    fc.check_chunk_route(lib, B, **size)


@pytest.mark.parametrize('size', SIZES[2:], ids=IDS[2:])
def test_prediction_behind_the_fits_tail(lib, size):
    # (N = 1024 only: at Np = 384 the one-output fit is a single worker launch and does not return before its tail)
    fc.check_behind_tail(lib, **size)


@pytest.mark.parametrize('size', SIZES[2:], ids=IDS[2:])
def test_fused_fit_predict(lib, size):
    fc.check_fused_fit_predict(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_mean_from_persistent_variance_product(lib, size):
    fc.check_fused_mean(lib, **size)


@pytest.mark.parametrize('B', [3, 33, 256])
@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_predict_sens_hessian(lib, size, B):
    fc.check_sens(lib, B, **size)


@pytest.mark.parametrize('d', [1, 9, 16])
def test_input_dimension_edges(lib, d):
    fc.check_edges(lib, B=9, **fc.EDGE_SIZES[d])


@pytest.mark.parametrize('kind', ['const', 'linear', 'polynomial'])
def test_prior_mean_functions(lib, kind):
    fc.check_edges(lib, B=33, **fc.PRIOR_SIZES[kind])


@pytest.mark.parametrize('size', SMALL, ids=SMALL_IDS)
def test_rollout_first_step(lib, size):
    fc.check_rollouts(lib, stride=4, **size)
