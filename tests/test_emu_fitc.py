"""CPU tier: gpmpc_sparse_fitc and GP.sparse on the emulated build of the unmodified HIP sources (tests/emu).  Sizes: the
smallest at which the paths differ -- N = 200, M = 70 (both off multiples of 64, M across two 64-blocks; predict_chunk = 64
gives four chunks, the last one ragged), N = 150, M = 64 with d = 9 (the second d-template family) and N = M = 130 (every
point inducing, sn = 0.1).  The checks live in fitc_cases.py; the GPU tier runs the same ones."""
import os
import subprocess

import pytest

import fitc_cases as fc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [dict(N=200, M=70, d=4, Ny=2, inducing='greedy'), dict(N=150, M=64, d=9, Ny=3), dict(N=130, M=130, d=4, Ny=1, sn=0.1)]
IDS = ['N200M70greedy', 'N150M64d9', 'N130all']


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_truth(emu, size):
    fc.check_truth(emu, **size)


def test_emu_truth_multi_chunk(emu):
    fc.check_truth(emu, chunk=64, **SIZES[0])


def test_emu_truth_unfitted_source(emu):
    fc.check_truth(emu, fitted=False, **SIZES[1])


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_emu_sparse_handle_is_an_ordinary_model(emu, size):
    fc.check_ordinary_model(emu, **size)


@pytest.mark.parametrize('size', SIZES[:2], ids=IDS[:2])
def test_emu_fitted_and_unfitted_source_agree_bitwise(emu, size):
    fc.check_fitted_and_unfitted_source(emu, **size)


def test_emu_argument_errors_leave_the_source_usable(emu):
    fc.check_argument_errors(emu, **SIZES[0])


def test_emu_sparse_handle_is_predict_only(emu):
    fc.check_predict_only(emu, **SIZES[0])


def test_emu_python_sparse(emu, tmp_path):
    fc.check_python(emu, tmp_path)
