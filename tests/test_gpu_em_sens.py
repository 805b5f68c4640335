"""GPU tier (-m gpu): the exact-moment Jacobians (gpmpc_predict_em_sens) against their longdouble value on fixed inputs --
every case of em_sens_cases.CASES -- and the routes of that entry point (host pointers beyond the packed block, device
pointers, far inputs) on a real MI355X.  The checks live in em_sens_cases.py; the emulator tier
(tests/test_emu_em_sens.py) runs the same ones less the three cases an emulated call is slow at."""
import pytest

import em_sens_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('label', list(ec.CASES))
def test_em_sens_fixed_input(lib, label):
    ec.check_case(lib, label)


def test_em_sens_unpacked_host(lib):
    ec.check_unpacked_host(lib)


def test_em_sens_device_pointers(lib):
    ec.check_device_pointers(lib)


def test_em_sens_far_inputs(lib):
    ec.check_far_inputs(lib)
