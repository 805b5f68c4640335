"""CPU tier: gpmpc_append_select and GP.update_data_select on the emulated build of the unmodified HIP sources (tests/emu).
Sizes: the smallest at which the paths differ -- N and n off multiples of 64, n across more than one 64-row workgroup, both
d-template families (d = 4 and d = 9), every candidate picked (k = n), k = 1.  The checks live in select_cases.py; the GPU
tier runs the same ones."""
import os
import subprocess

import pytest

import select_cases as sc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [dict(N=100, n=70, k=20, d=4, Ny=2), dict(N=150, n=130, k=64, d=9, Ny=3), dict(N=100, n=70, k=70, d=4, Ny=1, sn=0.1)]
IDS = ['N100k20', 'N150k64d9', 'N100k70all']


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_picks_gains_and_model(emu, size):
    sc.check_picks_gains_model(emu, **size)


def test_emu_single_pick(emu):
    sc.check_single_pick(emu, **SIZES[0])


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_selection_only_leaves_the_model_alone(emu, size):
    sc.check_selection_only(emu, **size)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_early_stop(emu, size):
    sc.check_early_stop(emu, **size)


def test_emu_degenerate_candidates(emu):
    sc.check_degenerate(emu)


def test_emu_mean_function(emu):
    sc.check_mean_function(emu)


def test_emu_argument_errors_leave_the_handle_usable(emu):
    sc.check_argument_errors(emu)


def test_emu_python_update_data_select(emu):
    sc.check_python(emu)
