"""CPU tier: gpmpc_remove, GP.remove_data and GP.update_data_window on the emulated build of the unmodified HIP sources
(tests/emu).  Sizes: the smallest at which the paths differ -- N = 150, n = 40 scattered (Np shrinks from 192 to 128, the
64-wide item kernels), N = 200, n = 70 oldest (d = 9, three outputs, two passes), N = 129, n = 1 (the padding vanishes, the
4-wide kernels), N = 70, n = 3 (one panel only) and n = 10 (the 16-wide kernels).  The checks live in remove_cases.py; the
GPU tier runs the same ones."""
import os
import subprocess

import pytest

import remove_cases as rc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

VS_FIT = [dict(N=150, n=40, kind='scattered', d=4, Ny=2), dict(N=200, n=70, kind='oldest', d=9, Ny=3),
          dict(N=129, n=1, kind='oldest', d=4, Ny=2), dict(N=70, n=3, kind='scattered', d=4, Ny=2),
          dict(N=150, n=1, kind='single', d=4, Ny=2), dict(N=150, n=40, kind='run', d=4, Ny=2),
          dict(N=150, n=10, kind='scattered', d=4, Ny=2, sn=0.1), dict(N=150, n=40, kind='oldest', d=4, Ny=2)]


def _id(s):
    return f"N{s['N']}n{s['n']}{s['kind']}"


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('size', VS_FIT, ids=_id)
def test_emu_remove_matches_a_fit_on_the_remaining_rows(emu, size):
    rc.check_vs_fit(emu, **size)


@pytest.mark.parametrize('size', [dict(N=150, n=40), dict(N=200, n=70, d=9, Ny=3)], ids=['N150n40', 'N200n70'])
def test_emu_trailing_indices_leave_the_leading_block_bitwise(emu, size):
    rc.check_trailing(emu, **size)


def test_emu_sliding_window(emu):
    rc.check_sliding_window(emu, N=150)


def test_emu_remove_then_append_the_same_rows(emu):
    rc.check_remove_then_append(emu, N=150, n=40)


def test_emu_remove_after_set_factors(emu):
    rc.check_after_set_factors(emu, N=150, n=40)


def test_emu_mean_function(emu):
    rc.check_mean_function(emu, N=150, n=40)


def test_emu_invK_is_rebuilt(emu):
    rc.check_invK(emu, N=150, n=40)


def test_emu_refit_branch_and_automatic_rule(emu):
    rc.check_refit_branch(emu, N=150, n=40)


def test_emu_argument_errors_leave_the_model_alone(emu):
    rc.check_argument_errors(emu, N=70)


def test_emu_python_remove_data_and_window(emu):
    rc.check_python(emu)
