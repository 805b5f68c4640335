"""GPU tier (-m gpu): gpmpc_sparse_fitc and GP.sparse on a real MI355X.  Sizes: N = 5000, M = 300, d = 5, three outputs with
predict_chunk = 1024 (five chunks, the last ragged) and in one chunk; N = 1024, M = 450, two outputs, sn = 0.1; N = 10000,
M = 256 on a source handle that is never fitted (a size no exact fit is asked for; half of the 20000 first planned: the
longdouble truth is a plain loop, 4e8 extended multiply-adds for this case, and has to stay at a few seconds).  The checks live in fitc_cases.py; the
emulator tier runs the same ones at toy size.  The distances of the truth gates go to profiles/fitc_digits.txt."""
import os

import pytest

import fitc_cases as fc

pytestmark = pytest.mark.gpu

SIZES = [dict(N=5000, M=300, d=5, Ny=3), dict(N=1024, M=450, d=4, Ny=2, sn=0.1), dict(N=10000, M=256, d=4, Ny=1)]
IDS = ['N5000M300', 'N1024M450', 'N10000M256']
DIGITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'fitc_digits.txt')


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    yield lib
    if fc.DIGITS:                         # the record of this run (no dates, no host names: the same run writes the same file)
        try:
            with open(DIGITS_FILE, 'w') as f:
                f.write('tests/test_gpu_fitc.py on ' + lib.device_name() + '\n')
                f.write('distance from the longdouble FITC value at 300 test points: mean in units of max|mean|, variance in units of sf^2\n')
                f.write(f'{"case":58s} {"mean device":>12s} {"mean numpy":>12s} {"var device":>12s} {"var numpy":>12s}\n')
                for label, dm, nm, dv, nv in fc.DIGITS:
                    f.write(f'{label:58s} {dm:12.2e} {nm:12.2e} {dv:12.2e} {nv:12.2e}\n')
        except OSError:
            pass


def test_truth_multi_chunk(lib):
    fc.check_truth(lib, chunk=1024, **SIZES[0])


@pytest.mark.parametrize('size', SIZES[:2], ids=IDS[:2])
def test_truth_single_chunk(lib, size):
    fc.check_truth(lib, **size)


def test_truth_unfitted_source_large_n(lib):
    fc.check_truth(lib, fitted=False, **SIZES[2])


@pytest.mark.parametrize('size', SIZES[:2], ids=IDS[:2])
def test_sparse_handle_is_an_ordinary_model(lib, size):
    fc.check_ordinary_model(lib, **size)


def test_fitted_and_unfitted_source_agree_bitwise(lib):
    fc.check_fitted_and_unfitted_source(lib, **SIZES[1])


def test_argument_errors_leave_the_source_usable(lib):
    fc.check_argument_errors(lib, **SIZES[1])


def test_sparse_handle_is_predict_only(lib):
    fc.check_predict_only(lib, **SIZES[1])


def test_python_sparse(lib, tmp_path):
    fc.check_python(lib, tmp_path)
