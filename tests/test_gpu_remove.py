"""GPU tier (-m gpu): gpmpc_remove, GP.remove_data and GP.update_data_window on a real MI355X.  Sizes: N = 1024, n = 64
oldest (d = 5, three outputs: every panel is reflected), N = 2500, n = 200 scattered (two outputs, sn = 0.1: four passes, Np
shrinks), N = 1100, n = 1 and N = 100, n = 60 (the refit branch under the automatic rule).  The checks live in
remove_cases.py; the emulator tier runs the same ones at toy size."""
import pytest

import remove_cases as rc

pytestmark = pytest.mark.gpu

VS_FIT = [dict(N=1024, n=64, kind='oldest', d=5, Ny=3), dict(N=2500, n=200, kind='scattered', d=4, Ny=2, sn=0.1),
          dict(N=1100, n=1, kind='single', d=4, Ny=2), dict(N=1024, n=64, kind='run', d=5, Ny=3)]


def _id(s):
    return f"N{s['N']}n{s['n']}{s['kind']}"


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('size', VS_FIT, ids=_id)
def test_remove_matches_a_fit_on_the_remaining_rows(lib, size):
    rc.check_vs_fit(lib, **size)


def test_trailing_indices_leave_the_leading_block_bitwise(lib):
    rc.check_trailing(lib, N=1024, n=64, d=5, Ny=3)


def test_sliding_window(lib):
    rc.check_sliding_window(lib, N=1100)


def test_remove_then_append_the_same_rows(lib):
    rc.check_remove_then_append(lib, N=1100, n=40)


def test_remove_after_set_factors(lib):
    rc.check_after_set_factors(lib, N=1100, n=40)


def test_mean_function(lib):
    rc.check_mean_function(lib, N=1100, n=40)


def test_invK_is_rebuilt(lib):
    rc.check_invK(lib, N=1100, n=40)


def test_refit_branch_and_automatic_rule(lib):
    rc.check_refit_branch(lib, N=1100, n=40)


def test_automatic_rule_refits_small_models(lib):
    rc.check_automatic_refits(lib, N=100, n=60)


def test_argument_errors_leave_the_model_alone(lib):
    rc.check_argument_errors(lib, N=1100)


def test_python_remove_data_and_window(lib):
    rc.check_python(lib)
