"""GPU tier (-m gpu): gpmpc_append_select and GP.update_data_select on a real MI355X.  Sizes: N = 1024 (k = 100: the strip
branch of the append, three outputs, d = 5), N = 2500 (two outputs, sn = 0.1) and N = 100 with every candidate picked (the
refit branch).  The checks live in select_cases.py; the emulator tier runs the same ones at toy size."""
import pytest

import select_cases as sc

pytestmark = pytest.mark.gpu

SIZES = [dict(N=1024, n=300, k=100, d=5, Ny=3), dict(N=2500, n=200, k=64, d=4, Ny=2, sn=0.1),
         dict(N=100, n=70, k=70, d=4, Ny=1, sn=0.1)]
IDS = ['N1024strip', 'N2500', 'N100refit']


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_picks_gains_and_model(lib, size):
    sc.check_picks_gains_model(lib, **size)


def test_single_pick(lib):
    sc.check_single_pick(lib, **SIZES[0])


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_selection_only_leaves_the_model_alone(lib, size):
    sc.check_selection_only(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_early_stop(lib, size):
    sc.check_early_stop(lib, **size)


def test_degenerate_candidates(lib):
    sc.check_degenerate(lib)


def test_mean_function(lib):
    sc.check_mean_function(lib)


def test_argument_errors_leave_the_handle_usable(lib):
    sc.check_argument_errors(lib)


def test_python_update_data_select(lib):
    sc.check_python(lib)
