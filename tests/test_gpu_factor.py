"""GPU tier (-m gpu): the fit's factors of every execution of the factorisation, per 64 x 64 tile against their
extended-precision values, on a real MI355X -- at the smallest sizes where each execution engages (SEGR = 512, 224 workers,
two-level widths 8 and 14).  The checks, the measures, how the bars were derived and the table of cases and routes live in
factor_cases.py; the emulator tier (test_emu_factor.py) runs the same checks.  d = 6, seed 1234, sn = 1e-2 (N = 520 also at
1e-3, the jitter case at 1e-8).  Each test is one fit (two in the jitter and append cases), a get_factors and a gpmpc_nll at
N <= 2000; the yardstick of a model is host work done once per process.

Seconds per case on the MI355X host, yardstick included (K_t, L_t, alpha_t, the tile products; a model's yardstick is formed
once and shared): N <= 520: 0.1 to 1.4;  N = 1000 / 1100: 0.8 to 3.9;  N = 1800 / 2000 (no L_t, named block rows): 4.6 / 4.8;
gpmpc_cholesky n = 1000: 6.3.  All 21 cases: 37 s.  On the development host the same yardsticks take 2 s (N = 520) to 9 s (N = 1000)."""
import pytest

import factor_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize('case', list(fc.CASES['gpu']))
def test_factor(lib, case):
    fc.run_case(lib, 'gpu', case)
