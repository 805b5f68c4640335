"""CPU tier: the exact-moment Jacobians (gpmpc_predict_em_sens) against their longdouble value on fixed inputs, and the
routes of that entry point (host pointers beyond the packed block, device pointers, far inputs), on the emulated build of the
unmodified HIP sources (tests/emu).  The checks and the cases live in em_sens_cases.py.
Not here, because the emulator takes more than 20 s for each: 'two inputs' (N = 555, B = 2, run twice: 24 s), 'DIAG only'
(N = 1100: 86 s) and "C3's dimensions" (N = 600, Ny = 6: 97 s, nearly all of it the emulated fit with K^-1).  The GPU tier
(tests/test_gpu_em_sens.py) runs all nine; profiles/em_sens_fixed_input_digits.txt has the emulator's figures for them as well."""
import os
import subprocess

import pytest

import em_sens_cases as ec
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = ['one tile', 'one real row in tile 2', 'ragged, Ny = 3, d = 1', '16-deep', '16-deep, full', 'wide Sigma']


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('label', CASES)
def test_emu_em_sens_fixed_input(emu, label):
    ec.check_case(emu, label)


def test_emu_em_sens_unpacked_host(emu):
    ec.check_unpacked_host(emu)


def test_emu_em_sens_device_pointers(emu):
    ec.check_device_pointers(emu)


def test_emu_em_sens_far_inputs(emu):
    ec.check_far_inputs(emu)
