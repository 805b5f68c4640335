"""GPU tier (-m gpu): gpmpc_rollout_multi_feedback and GP.rollout_closed_loop on a real MI355X, at the sizes of
test_rollout_multi_lockstep_matches_single_rollouts (N = 1024, Ny = 3, d = 5, T = 8 and N = 2500, Ny = 2, d = 4, T = 4).
The checks live in rollout_feedback_cases.py; the emulator tier runs the same ones at toy size."""
import pytest

import rollout_feedback_cases as rc

pytestmark = pytest.mark.gpu

SIZES = [dict(N=1024, Ny=3, d=5, T=8), dict(N=2500, Ny=2, d=4, T=4)]


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'N{s["N"]}')
def test_one_closed_trajectory_is_bitwise_rollout_feedback(lib, size):
    rc.check_single_closed(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'N{s["N"]}')
def test_all_open_is_bitwise_rollout_multi(lib, size):
    rc.check_all_open(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'N{s["N"]}')
def test_mixed_closed_and_open_call(lib, size):
    rc.check_mixed(lib, **size)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'N{s["N"]}')
def test_closed_trajectory_does_not_depend_on_position_or_neighbours(lib, size):
    rc.check_position_invariance(lib, **size)


def test_closed_loop_against_oracle_tank(lib, tank):
    rc.check_closed_loop_vs_oracle_tank(lib, tank, T=8)


def test_closed_loop_against_oracle_synthetic(lib):
    rc.check_closed_loop_vs_oracle_synthetic(lib)


def test_closed_loop_more_than_64_trajectories(lib):
    rc.check_closed_loop_split(lib)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'N{s["N"]}')
def test_model_fitted_without_invK(lib, size):
    rc.check_without_invK(lib, **size)


def test_argument_errors_leave_the_handle_usable(lib):
    rc.check_argument_errors(lib, N=1024, Ny=3, d=5, T=8)
