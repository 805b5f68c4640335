"""CPU tier: gpmpc_rollout_multi_feedback and GP.rollout_closed_loop on the emulated build of the unmodified HIP sources
(tests/emu), at N = 150, Ny = 2, d = 4, T = 5.  The checks live in rollout_feedback_cases.py; the GPU tier runs the same ones."""
import os
import subprocess

import pytest

import rollout_feedback_cases as rc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


def test_emu_one_closed_trajectory_is_bitwise_rollout_feedback(emu):
    rc.check_single_closed(emu)


def test_emu_all_open_is_bitwise_rollout_multi(emu):
    rc.check_all_open(emu)
    rc.check_all_open(emu, moment='old_ME')


def test_emu_mixed_closed_and_open_call(emu):
    rc.check_mixed(emu)


def test_emu_closed_trajectory_does_not_depend_on_position_or_neighbours(emu):
    rc.check_position_invariance(emu)


def test_emu_closed_loop_against_oracle_tank(emu, tank):
    rc.check_closed_loop_vs_oracle_tank(emu, tank)


def test_emu_closed_loop_against_oracle_synthetic(emu):
    rc.check_closed_loop_vs_oracle_synthetic(emu)


def test_emu_closed_loop_more_than_64_trajectories(emu):
    rc.check_closed_loop_split(emu)


def test_emu_model_fitted_without_invK(emu):
    rc.check_without_invK(emu)


def test_emu_argument_errors_leave_the_handle_usable(emu):
    rc.check_argument_errors(emu)
