"""GPU tier (-m gpu): the parity tests proper.  Everything goes through the C ABI of the
hipcc-built product library on a real MI355X and is compared with the oracle on identical inputs."""
import time

import numpy as np
import pytest

import gp_oracle as go
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from gp_mpc_amd._lib import get_lib
    lib = get_lib()                       # raises if libgpmpc_hip.so is missing: no fallback
    assert lib.device_count() >= 1
    return lib


def test_mfma_selftest(lib):
    layout, tflops = lib.mfma_selftest(0)
    print(f'\n[mfma] device={lib.device_name(0)} f64 16x16x4 layout={layout} issue-bound rate={tflops:.1f} TFLOP/s')
    assert layout in (0, 1)
    assert tflops > 10.0


def test_dgemm_large_tile(lib):
    pc.check_dgemm_large_tile(lib)


def test_forced_tiles(lib, tank):
    pc.check_forced_tiles(lib, tank)


def test_dgemm(lib):
    pc.check_dgemm(lib, sizes=((70, 33, 50), (128, 128, 64), (200, 130, 96), (1000, 900, 512), (2048, 2048, 256)))


def test_cholesky_small(lib):
    pc.check_cholesky(lib, sizes=(64, 100, 192, 256, 1000))


def test_cholesky_4096_matches_cpu(lib):
    """north_star: 'Cholesky matching CPU to 1e-10 rel' at the C2 size."""
    p = go.synthetic_problem(4096, 6, 1, 1, seed=1234)
    K = go.gram(p['X'], p['hyper'][0, :6], 1.0, 1e-4)
    L, Li, info = lib.cholesky(K, want_inverse=True)
    Lr = np.linalg.cholesky(K)
    assert info == 0
    assert pc.relF(L, Lr) <= 1e-10
    assert np.linalg.norm(L @ L.T - K) / np.linalg.norm(K) <= 1e-14
    assert np.abs(Li @ Lr - np.eye(4096)).max() <= 1e-9


def test_tank_model(lib, tank):
    pc.check_model_fixture(lib, tank, tolL=1e-10, tol_nll=1e-10)


def test_car_model_cond_7e10_bars_5e10_L_1e7_nll(lib, car):
    """The reference's car model has cond(K) up to 7e10: numpy re-deriving its own stored factor on another
    LAPACK build is at 8e-11, so L is held to 5e-10 and the (cond-limited) NLL to 1e-7 here; the well-conditioned
    synthetic sets below carry the plain 1e-10 bars."""
    pc.check_model_fixture(lib, car, tolL=5e-10, tol_nll=1e-7)


def test_gp_class_strict_bars_on_well_conditioned_model(lib):
    pc.check_gp_class_strict(lib)


def test_synthetic_strict(lib):
    pc.check_synthetic(lib, N=1024, d=6, Ny=2, B=300, sn=0.1, strict_rel=True)


def test_synthetic_default_noise(lib):
    pc.check_synthetic(lib, N=1500, d=8, Ny=3, B=1000, sn=1e-2, strict_rel=False)


def test_predict_behind_tail_c2_size(lib):
    """The first large prediction behind a fit runs next to the tail of L^-1 (cross-covariances on a second queue while the
    last row panel is inverted, alpha and the mean on the workers' queue next to the variance product): same bits as the
    plain route, oracle bars; at the C2 size and around it."""
    pc.check_predict_behind_tail(lib, N=4096, d=6, B=10000, sn=0.1, strict=True, repeats=3)
    pc.check_predict_behind_tail(lib, N=4096, d=6, B=1000, sn=1e-2, strict=False, seed=1234)
    pc.check_predict_behind_tail(lib, N=2048, d=4, B=700, sn=0.1, mean_only_second=True)
    pc.check_predict_behind_tail(lib, N=3000, d=5, B=900, sn=0.1)
    pc.check_predict_behind_tail(lib, N=4100, d=6, B=600, sn=0.1)
    pc.check_predict_behind_tail(lib, N=500, d=6, B=200, sn=0.1, expect_overlap=None)


@pytest.mark.parametrize('version', ['3.4.5', '3.6.3'])
def test_callback_classes_execute_under_stub_casadi(lib, version):
    """the casadi.Callback subclasses (single node = GP.__predict's signature gp_class.py:212-224, and all
    shooting nodes of mpc_class.py:361-423 in one call) driven through CasADi's Callback protocol by tests/stub_casadi.py,
    both Jacobian conventions; values vs OracleGP.predict, Jacobians vs central differences of the oracle."""
    import stub_casadi
    pc.check_callback_classes(lib, stub_casadi, version, N=200, Ny=3, Nu=2, Nt=4)


def test_variance_persistent_schedule(lib):
    """vargemm_persist.hpp at the C2 size (512 slots, 2528 tiles) and on a ragged two-output shape: same bits as the
    one-tile-per-workgroup launch, oracle bars."""
    pc.check_variance_persistent(lib, N=4096, d=6, Ny=1, B=10000)
    pc.check_variance_persistent(lib, N=1500, d=4, Ny=2, B=3000)


def test_jitter_rule(lib, train_small):
    pc.check_jitter_rule(lib, train_small)


def test_nll_gradient(lib, tank):
    pc.check_nll_gradient(lib, tank)


def test_c2_full_size_vs_oracle_and_properties(lib):
    """BASELINE config C2 (N=4096, d=6, 10k predictions) against the oracle on the same inputs,
    plus size-independent properties: batch invariance (bitwise), 0 <= var <= sf^2, chunking."""
    from gp_mpc_amd._lib import Handle
    t0 = time.time()
    r = pc.check_synthetic(lib, N=4096, d=6, Ny=1, B=10000, sn=1e-2, strict_rel=False)
    print(f'\n[C2] full-size oracle comparison took {time.time() - t0:.1f} s')
    h = Handle(lib, r['X'], r['Y'])
    h.fit(r['H'])
    mean, var = r['mean'], r['var']
    m2, v2 = h.predict_mean_var(r['Z'][:777])
    # other batch size -> other GEMM tile / summation order for the variance and, since r04, for the mean as well: the large
    # batch takes it from the persistent variance product's fused reduction (L^-1 ks)^T (L^-1 y), the small one from ks^T alpha
    sc = pc.mean_scale(r['X'], r['Z'][:777], r['H'], go.fit(r['X'], r['Y'], r['H'], want_invK=False)['alpha'])
    assert np.max(np.abs(m2 - mean[:777]) / sc) <= 1e-12
    assert np.max(np.abs(v2 - var[:777])) <= 1e-13
    m3, v3 = h.predict_mean_var(r['Z'])
    assert np.array_equal(m3, mean) and np.array_equal(v3, var)                 # run-to-run deterministic
    assert np.all(var > 0) and np.all(var <= 1.0 + 1e-12)
    mt, vt = h.predict_mean_var(r['X'][:512])                                   # at training inputs
    assert np.max(np.abs(mt[:, 0] - r['Y'][:512, 0])) < 0.2 and np.all(vt < 1e-3)
    h.close()


def test_c2_full_size_rel_to_max_and_floored_pointwise_bars(lib):
    """SURVEY 8c / north_star "within 1e-10 rel": the C2 size with sn = 0.1 (well conditioned).  What is gated, by name
    (check_synthetic strict_rel, parity_cases.mean_bars): ||dL||_F / ||L||_F, the variance pointwise, |dNLL| / (|NLL| + N),
    and for the mean BOTH max|dmean| / max|mean| and the pointwise error with a floor of 1e-2 max|mean| (parity_cases.check_synthetic says why) -- all <= 1e-10;
    the unfloored pointwise figure (means that cross zero) is reported by bench.py, not gated."""
    t0 = time.time()
    pc.check_synthetic(lib, N=4096, d=6, Ny=1, B=10000, sn=0.1, strict_rel=True)
    print(f'\n[C2 strict] took {time.time() - t0:.1f} s')


def test_moment_methods(lib, tank):
    pc.check_moment_methods(lib)
    pc.check_moment_methods(lib, tank)


def test_worker_path_odd_size(lib):
    # Np = 4032 = 63 blocks: tile-owner workers in two launches (32 + 31 blocks), tree with an unbalanced root
    pc.check_synthetic(lib, N=4000, d=6, Ny=1, B=200, sn=1e-2, strict_rel=False)
    # Np = 4160 = 65 blocks: 2079 tiles, ten slots of 223 owners hold them (r03; the nine-slot kernel below does not:
    # chain kernel + flagged GEMM launches)
    pc.check_synthetic(lib, N=4100, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)
    # Np = 4288 = 67 blocks: 2210 tiles, the most 223 owners hold (ten each); Np = 4352: one block more -> GEMM launches
    pc.check_synthetic(lib, N=4280, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)
    pc.check_synthetic(lib, N=4300, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)


def test_worker_path_without_courier(lib):
    # the nine-slot instantiation of the worker kernel (tile owners make the chain's hand-off tiles themselves)
    lib.set_tuning('worker_courier', 0)
    try:
        pc.check_synthetic(lib, N=4096, d=6, Ny=1, B=100, sn=1e-2, strict_rel=False)
        pc.check_synthetic(lib, N=4000, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)
        pc.check_synthetic(lib, N=4100, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)
    finally:
        lib.set_tuning('worker_courier', -1)


def test_worker_path_with_release_fence_handoffs(lib):
    # the r01-r03 form of every hand-off inside the chained factorisation (plain stores + agent-scope release) stays selectable
    lib.set_tuning('handoff_write_through', 0)
    try:
        pc.check_synthetic(lib, N=4096, d=6, Ny=1, B=100, sn=1e-2, strict_rel=False)
        pc.check_synthetic(lib, N=4100, d=6, Ny=1, B=50, sn=1e-2, strict_rel=False)
    finally:
        lib.set_tuning('handoff_write_through', -1)


def test_small_batch_chunks(lib):
    pc.check_small_batch_chunks(lib, N=2500, d=6, Ny=3)


def test_timeout_fallback(lib, capfd):
    pc.check_timeout_fallback(lib, N=1500)
    assert 'timed out on a hand-off' in capfd.readouterr().err


def test_append(lib):
    pc.check_append(lib, N0=300, n=10)
    pc.check_append(lib, N0=250, n=70)
    pc.check_append(lib, N0=2000, n=90, d=6, Ny=1, sn=1e-2)


def test_append_series_through_the_block_list(lib):
    pc.check_append_series(lib)


def test_append_after_set_factors_and_rollback(lib):
    pc.check_append_after_set_factors(lib)
    pc.check_append_after_set_factors(lib, N0=2000, n=90, d=6, Ny=1)
    pc.check_append_rollback(lib)


def test_sensitivities(lib, tank, car):
    pc.check_sensitivities(lib, tank)
    pc.check_sensitivities(lib, car, nprobe=20)
    pc.check_sensitivities_batches(lib)


def test_gp_class(lib, tank, tmp_path):
    pc.check_gp_class(lib, tank, tmp_path)


def test_training(lib, train_small):
    pc.check_training(lib, train_small)


def test_em_sens(lib):
    pc.check_em_sens(lib)
    pc.check_em_sens(lib, N=600, d=8, Ny=6, B=3, seed=4)          # C3's output / input dimensions
    pc.check_em_sens(lib, N=100, d=1, Ny=3, B=2, seed=7)          # one input dimension
    pc.check_em_sens(lib, N=47, d=7, Ny=4, B=1, seed=8)           # ragged, nearly the full cross-term depth
    pc.check_em_sens(lib, N=150, d=9, Ny=2, B=2, seed=9)          # d > 8: the 16-deep instantiation of the kernels
    pc.check_em_sens(lib, N=200, d=16, Ny=3, B=1, seed=10)        # the largest input dimension the library takes
    pc.check_em_sens(lib, N=90, d=12, Ny=1, B=2, seed=11)


def test_callback_blocks(lib):
    pc.check_callback_blocks(lib)
    pc.check_callback_blocks(lib, N=500, Ny=6, Nu=2, seed=3)


def test_callback_all_nodes_in_one_call(lib):
    """make_batched_predict_callback's numeric core: Nt nodes per call, block-diagonal Jacobian (dense 3.4-style stacking
    and per-pair triplets) against central differences, all five methods."""
    pc.check_callback_batched(lib)
    pc.check_callback_batched(lib, N=400, Ny=4, Nu=2, Nt=6, seed=5)


def test_feedback_rollout(lib, tank):
    pc.check_feedback_rollout(lib, tank, T=8)


def test_mean_functions(lib):
    pc.check_mean_functions(lib)
    pc.check_mean_functions(lib, N=700, d=6, Ny=3, seed=5)


def test_training_native(lib, train_small):
    pc.check_training_native(lib, train_small)


def test_random_shapes(lib):
    pc.check_random_shapes(lib, n_cases=25, nmax=700)


def test_edge_cases(lib):
    pc.check_edge_cases(lib)


def test_c3_size_properties(lib):
    """BASELINE config C3 size (6 outputs, N=8192, d=8): too large for the oracle in seconds, so
    size-independent properties: mean at training inputs satisfies K alpha = y exactly
    (mean(x_i) = y_i - sn^2 alpha_i), 0 < var <= sf^2, ME/TA/EM agree for a vanishing input covariance, EM covariance symmetric PSD."""
    from gp_mpc_amd._lib import Handle
    p = go.synthetic_problem(8192, 8, 6, 16, seed=1234, sn=1e-2)
    h = Handle(lib, p['X'], p['Y'])
    assert np.all(h.fit(p['hyper'], want_invK=True) == 0)
    mt, vt = h.predict_mean_var(p['X'][:64])
    al = h.get_factors(chol=False)['alpha']
    sn2 = p['hyper'][:, 9] ** 2
    resid = mt - (p['Y'][:64] - sn2[None, :] * al[:, :64].T)
    assert np.max(np.abs(resid)) <= 1e-8 * np.abs(al).max()      # (K_se + sn^2 I) alpha = y, cond-scaled
    assert np.all(vt > 0) and np.all(vt < 1.0)
    Z = p['Z'][:4]
    m0, v0 = h.predict_mean_var(Z)
    tiny = np.tile(np.eye(8) * 1e-12, (4, 1, 1))
    mT, cT = h.predict('TA', Z, tiny)
    mE, cE = h.predict('EM', Z, tiny)
    assert np.allclose(mT, m0, rtol=0, atol=1e-12) and np.allclose(mE, m0, rtol=1e-6, atol=1e-6)
    assert np.allclose(np.einsum('baa->ba', cT), v0, rtol=1e-6, atol=1e-10)   # + J (1e-12 I) J^T
    assert np.allclose(np.einsum('baa->ba', cE), v0, rtol=0, atol=1e-4)    # N^2-term sum against K^-1: cancellation-limited
    mS, cS = h.predict('EM', Z, p['Sigma'][:4])
    for b in range(4):
        assert np.array_equal(cS[b], cS[b].T) and np.linalg.eigvalsh(cS[b]).min() > -1e-8
    h.close()


def test_rollout_replay(lib):
    pc.check_rollout_replay(lib)


def test_io_pack_boundary(lib):
    pc.check_io_pack_boundary(lib)


def test_wide_inputs(lib):
    pc.check_wide_inputs(lib)


def test_training_active_bound(lib, train_small2):
    pc.check_training_active_bound(lib, train_small2)


def test_training_beats_failed_reference_search(lib, train_small3):
    pc.check_training_beats_failed_reference_search(lib, train_small3)


def test_training_never_worse(lib):
    pc.check_training_never_worse(lib, n_cases=10)


@pytest.mark.gpu
def test_set_factors_then_persistent_mean(lib):
    pc.check_set_factors_persistent_mean(lib)


def test_old_me_reference_pin(lib, tank, car, old_me_pins):
    pc.check_old_me_reference_pin(lib, tank, old_me_pins['tank'])
    pc.check_old_me_reference_pin(lib, car, old_me_pins['car'])


def test_em_pair_sum_chunks(lib):
    pc.check_em_chunks(lib)


@pytest.mark.parametrize('name', ['tank', 'car'])
def test_ta_and_jacobian_match_reference_run_pin(lib, name, request, ta_pins):
    """a9 J / a10 TA against reference-run outputs (tests/golden/{tank,car}_ta.npz), through gpmpc_predict_jac."""
    pc.check_ta_reference_pin(lib, request.getfixturevalue(name), ta_pins[name], name)


@pytest.mark.parametrize('name', ['train_small', 'em_model2'])
def test_exact_moments_match_reference_run_quadrature(lib, name, em_pins):
    """a11 EM against quadrature of the reference's own predictor on reference-trained models (1e-12 abs on em_model2)."""
    pc.check_em_reference_pin(lib, *em_pins[name], name)


def test_reference_written_model_file_loads_and_round_trips(lib, ref_written, tmp_path):
    pc.check_reference_written_model(lib, *ref_written, tmp_path)


def test_fused_fit_predict_same_bits_as_two_calls(lib):
    """gpmpc_fit_predict_mean_var at the C2 size and around it: bitwise the two calls' mean / variance / factors, oracle bars;
    the jitter retry repeats the prediction behind the repeated factorisation."""
    pc.check_fused_fit_predict(lib, N=4096, d=6, B=10000, repeats=3)
    pc.check_fused_fit_predict(lib, N=4096, d=6, B=1000, sn=1e-2, seed=1234)
    pc.check_fused_fit_predict(lib, N=3000, d=5, B=900)
    pc.check_fused_fit_predict(lib, N=2048, d=4, B=700)
    pc.check_fused_fit_predict(lib, N=1500, d=4, B=600, Ny=2)
    pc.check_fused_fit_predict(lib, N=1000, d=4, B=300, jitter_case=True, repeats=1)
    pc.check_fused_fit_predict(lib, N=500, d=6, B=40, expect_fused=False)


def test_rollout_multi_lockstep_matches_single_rollouts(lib):
    """gpmpc_rollout_multi: one pass over the factors per time step for all trajectories / methods."""
    pc.check_rollout_multi(lib, N=1024, Ny=3, d=5, T=8)
    pc.check_rollout_multi(lib, N=2500, Ny=2, d=4, T=4, methods=('ME', 'TA', 'EM'))


@pytest.mark.parametrize('sn', [1e-2, 0.1])
def test_c2_mean_is_as_close_to_the_extended_precision_value_as_numpy(lib, sn):
    """the C2 mean against a longdouble evaluation (iteratively refined alpha): the device's maximum and rms error
    gated at twice the fp64 oracle's own distance from that value (or 1e-10 max|mean|); pointwise figures with the floor of
    1e-3 max|mean| printed for both sides."""
    t0 = time.time()
    r = pc.check_mean_against_extended_precision(lib, N=4096, d=6, B=10000, sn=sn)
    print(f'[mean digits sn={sn}] device {r["device"]:.2e} oracle {r["oracle"]:.2e} ({time.time() - t0:.0f} s)')


def test_em_covariance_is_as_close_to_the_extended_precision_value_as_numpy(lib):
    pc.check_em_against_extended_precision(lib, N=1024, d=8, Ny=2)


def test_far_points_and_zero_signal_variance(lib):
    pc.check_far_points(lib)
    pc.check_far_points(lib, N=2500, d=3, Ny=1)


def test_soak_chained_fits_without_a_handoff_timeout(lib):
    """400 consecutive C2-size fits + predictions on an otherwise idle GPU with the default hand-off settings
    (write-through stores, leafdone published behind the panel row's products): not one hand-off may time out, every
    factorisation must have taken the chained path, and the factors of the last fit are the first fit's bit for bit."""
    from gp_mpc_amd._lib import Handle
    p = go.synthetic_problem(4096, 6, 1, 512, seed=1234, sn=1e-2)
    h = Handle(lib, p['X'], p['Y'])
    h.fit(p['hyper'])
    f0 = h.get_factors()
    m0, v0 = h.predict_mean_var(p['Z'])
    for _ in range(400):
        assert np.all(h.fit(p['hyper']) == 0)
        m, v = h.predict_mean_var(p['Z'])
    f1 = h.get_factors()
    assert h.counter('handoff_timeouts') == 0 and h.counter('single_queue_factorisations') == 0, \
        (h.counter('handoff_timeouts'), h.counter('single_queue_factorisations'))
    assert np.array_equal(f0['chol'], f1['chol']) and np.array_equal(f0['alpha'], f1['alpha'])
    assert np.array_equal(m, m0) and np.array_equal(v, v0)
    h.close()


def test_gp_rollout_lockstep_route(lib):
    pc.check_gp_rollout_lockstep(lib, N=800, T=8)


# ---- exact moments against the longdouble value of FIXED inputs (the device's own K^-1): pc.em_fixed_input_gate --------
@pytest.mark.parametrize('N', [2048, 2049])
def test_em_fixed_input_around_the_pair_overlap(lib, N):
    """Ny = 2 at Np = 2048 (the a == b launch on the main queue) and Np = 2112 (on the aux queue next to the a != b launch,
    last tile 1/64 live)."""
    p = go.synthetic_problem(N, 8, 2, 1, seed=N, sn=1e-2)
    pc.check_em_fixed_input(lib, f'N={N} d=8 Ny=2', p['X'], p['Y'], p['hyper'], p['Z'], p['Sigma'])


def test_em_fixed_input_one_output(lib):
    """Ny = 1 at N = 4100: no a != b launch, no overlap."""
    p = go.synthetic_problem(4100, 8, 1, 1, seed=41, sn=1e-2)
    pc.check_em_fixed_input(lib, 'N=4100 d=8 Ny=1', p['X'], p['Y'], p['hyper'], p['Z'], p['Sigma'])


@pytest.mark.parametrize('d', [9, 16])
def test_em_fixed_input_16_deep_cross_term(lib, d):
    p = go.synthetic_problem(2500 + d, d, 2, 1, seed=d, sn=1e-2)
    pc.check_em_fixed_input(lib, f'N={2500 + d} d={d} Ny=2', p['X'], p['Y'], p['hyper'], p['Z'], p['Sigma'] * 30)


def test_em_fixed_input_schedules_where_every_tile_matters(lib):
    """Clustered training set (Q = O(1) in every tile), N = 3001: the a == b ranges (1, 2, 7, default, T - 1, T, > T) and
    strips and chunks (1, 3, 64 tiles, whole strips)."""
    X, Y, H, Z, S = pc.clustered_problem(3001, 4, 2, B=1)
    pc.check_em_fixed_input(lib, 'clustered N=3001 d=4 Ny=2', X, Y, H, Z, S, tunings=pc.em_schedule_tunings(3001))


def test_em_fixed_input_clamp_routing(lib):
    pc.check_em_fixed_input_clamp_routing(lib)


# ---- the multi-chunk paths of the predict family ('predict_chunk' / 'em_sens_chunk': pc.same_bits_as_slices + oracle bars) ----
def test_chunk_knobs_validation(lib):
    pc.check_chunk_knobs_validation(lib)


def test_chunked_mean_var(lib):
    pc.check_chunked_mean_var(lib)


def test_chunked_jac_copy_routes(lib):
    pc.check_chunked_jac_copy_routes(lib)


def test_chunked_methods(lib):
    pc.check_chunked_methods(lib)


def test_chunked_sens(lib):
    pc.check_chunked_sens(lib)


def test_chunked_device_pointers(lib):
    pc.check_chunked_device_pointers(lib)


def test_chunked_mean_function(lib):
    pc.check_chunked_mean_function(lib)


def test_em_sens_chunks(lib):
    pc.check_em_sens_chunks(lib)


def test_covar_chunks(lib):
    pc.check_covar_chunks(lib)


def test_sens_device_pointers(lib):
    pc.check_sens_device_pointers(lib)


def test_sens_unpacked_host(lib):
    pc.check_sens_unpacked_host(lib)


def test_covar_device_pointers(lib):
    pc.check_covar_device_pointers(lib)


def test_mean_var_null_outputs(lib):
    pc.check_mean_var_null_outputs(lib)


def test_chunk_routing(lib):
    pc.check_chunk_routing(lib, N=700, d=3, B=200)


def test_shipped_chunk_boundary_32768(lib):
    """The one multi-chunk case without the knob: B = 32768 + 100 at N = 100, Ny = 2 (about 70 MB of scratch)."""
    pc.check_shipped_chunk_boundary(lib)
