"""CPU tier: the fit's factors of every execution of the factorisation, per 64 x 64 tile against their extended-precision
values, on the emulated build of the unmodified HIP sources (tests/emu; SEGR = 128, 8 emulated CUs, two-level width 2).  The
checks, the measures, how the bars were derived and the table of cases and routes live in factor_cases.py; the GPU tier
(test_gpu_factor.py) runs the same checks at the sizes where the product's thresholds fall.  d = 4, seed 1234, sn = 1e-2 (one size
at 1e-3; the jitter case at 1e-8 and d = 6).  rho is measured on every lower tile at every size.

Seconds per case on the development host, yardstick and emulated fit together (the yardstick of a model is formed once and
shared by the cases on it): N = 60 / 150: under 1;  N = 330: 3 to 7;  N = 560: 10 to 24 (two outputs);  N = 700: 20;  N = 950: 60;
the module: 4 min 40 s, one minute of it the emulator build -- what test_emu_variance.py takes."""
import os
import subprocess

import pytest

import factor_cases as fc
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


@pytest.mark.parametrize('case', list(fc.CASES['emu']))
def test_emu_factor(emu, case):
    fc.run_case(emu, 'emu', case)
