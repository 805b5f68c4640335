"""GPU tier (-m gpu): the restart search of gpmpc_train_multistart against the oracle's replay of the same search on a real
MI355X.  Sizes: N = 300 (Np = 320: chain + flagged GEMM launches), N = 1000 (Np = 1024: two super-panels of 8 block columns,
the value-only trials leave L^-1 unformed), N = 1100 (Np = 1152: a ragged third super-panel; alone, the tile-owner workers
of gpmpc_nll), N = 1800 (Np = 1856: super-panels of 14 block columns).  The checks and the seeds' conditions live in
train_replay_cases.py; the emulator tier runs the same ones at toy size.  Most of a case's time is the oracle's."""
import pytest

import train_replay_cases as tr

pytestmark = pytest.mark.gpu

# start seeds per restart, chosen on the CPU so that the input conditions of train_replay_cases hold (they are asserted)
FLAGGED = dict(N=300, d=3, max_iter=3, useeds=(3, 5, 11, 12))
TWOLEVEL = dict(N=1000, d=4, max_iter=3, useeds=(1, 2, 3, 4, 5))
RAGGED = dict(N=1100, d=3, max_iter=2, useeds=(1, 2, 4))
WIDE = dict(N=1800, d=3, max_iter=2, useeds=(1, 2))
SUBSET = dict(N=1000, d=3, max_iter=2, useeds=(1, 2, 4, 0), jitter=True)
SPLIT = dict(N=300, d=3, max_iter=3, useeds=(3, 5, 12))
SINGLE = dict(N=1100, d=3, max_iter=2, useeds=(1,))
TWO_OUTPUTS = dict(N=300, d=3, Ny=2, max_iter=3, useeds=(11, 12, 14))
MEAN = dict(N=300, d=2, max_iter=3, useeds=(24, 25, 29))
PRIOR = dict(N=300, d=3, max_iter=3, prior=True, useeds=(6, 11, 12))


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


def test_flagged_execution_retained_path(lib):
    tr.check_replay(lib, **FLAGGED)


def test_twolevel_panels_value_only_skip(lib):
    tr.check_replay(lib, **TWOLEVEL)


def test_ragged_last_super_panel(lib):
    tr.check_replay(lib, **RAGGED)


def test_super_panel_width_14(lib):
    tr.check_replay(lib, **WIDE)


@pytest.mark.parametrize('persist', [-1, 0, 2], ids=['auto', 'scattered', 'persistent'])
def test_zmap_subset_and_jitter_slot_remap(lib, persist):
    tr.check_replay(lib, persist=persist, need_subset=True, **SUBSET)


def test_split_batches_no_retention(lib):
    tr.check_replay(lib, route='split', cap=2, **SPLIT)


def test_single_restart_worker_factorisation(lib):
    tr.check_replay(lib, route='single', **SINGLE)


def test_two_outputs(lib):
    tr.check_replay(lib, **TWO_OUTPUTS)


@pytest.mark.parametrize('mean', ['linear', 'polynomial'])
def test_mean_function(lib, mean):
    tr.check_replay(lib, mean=mean, **MEAN)


def test_hyper_prior(lib):
    tr.check_replay(lib, **PRIOR)
