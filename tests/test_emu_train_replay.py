"""CPU tier: the restart search of gpmpc_train_multistart against the oracle's replay of the same search, on the emulated build
of the unmodified HIP sources (tests/emu; two-level panels of 2 block columns there).  Sizes: N = 100 (Np = 128: chain +
flagged GEMM launches), N = 200 (Np = 256: two super-panels) and N = 300 (Np = 320: three super-panels, the last one ragged;
the value-only trials leave L^-1 unformed), N = 130 for the single-restart route.  The checks and the seeds' conditions live in
train_replay_cases.py; the GPU tier runs the same ones."""
import os
import subprocess

import pytest

import train_replay_cases as tr
from gp_mpc_amd._lib import GpmpcLib

HERE = os.path.dirname(os.path.abspath(__file__))

# start seeds per restart, chosen on the CPU so that the input conditions of train_replay_cases hold (they are asserted)
FLAGGED = dict(N=100, d=2, max_iter=3, useeds=(31, 43, 46))
TWOLEVEL = dict(N=300, d=3, max_iter=3, useeds=(3, 5, 12))
SUBSET = dict(N=200, d=3, max_iter=3, useeds=(25, 3, 0), jitter=True)


@pytest.fixture(scope='module')
def emu():
    subprocess.check_call([os.path.join(HERE, 'emu', 'build_emu.sh')], stdout=subprocess.DEVNULL)
    return GpmpcLib(os.path.join(HERE, 'emu', '_build', 'libgpmpc_emu.so'))


def test_emu_flagged_execution_retained_path(emu):
    tr.check_replay(emu, **FLAGGED)


def test_emu_first_step_alone(emu):
    tr.check_replay(emu, **dict(FLAGGED, max_iter=1))


def test_emu_twolevel_panels_ragged_value_only_skip(emu):
    tr.check_replay(emu, **TWOLEVEL)


@pytest.mark.parametrize('persist', [-1, 0, 2], ids=['auto', 'scattered', 'persistent'])
def test_emu_zmap_subset_and_jitter_slot_remap(emu, persist):
    tr.check_replay(emu, persist=persist, need_subset=True, **SUBSET)


def test_emu_split_batches_no_retention(emu):
    tr.check_replay(emu, route='split', cap=2, **SUBSET)


def test_emu_single_restart(emu):
    tr.check_replay(emu, route='single', N=130, d=4, max_iter=3, seed=2, useeds=(6,))


def test_emu_two_outputs(emu):
    tr.check_replay(emu, N=100, d=2, Ny=2, max_iter=3, useeds=(25, 31, 43))


@pytest.mark.parametrize('mean,useeds', [('linear', (31, 43, 46)), ('polynomial', (31, 43, 46))], ids=['linear', 'polynomial'])
def test_emu_mean_function(emu, mean, useeds):
    tr.check_replay(emu, N=100, d=2, max_iter=3, mean=mean, useeds=useeds)


def test_emu_hyper_prior(emu):
    tr.check_replay(emu, N=100, d=2, max_iter=3, prior=True, useeds=(25, 31, 56))
