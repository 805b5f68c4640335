// api_select.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: gpmpc_append_select -- greedy max-variance choice among candidate points (select_kernels.hpp), then gpmpc_append
// of the chosen rows.
// ------------------------------------------------------------------------------------------------
// The selection alone: picks[0 .. kout), gains[0 .. kout).  Everything n x n stays on the device.
static int select_greedy(gpmpc_gp* h, int n, const double* Xcand, int k, double min_gain, std::vector<int>& picks,
                         std::vector<double>& gains, int& kout) {
    CHK(ensure_scratch(h, n));
    const Ctx cx = h->cx();
    const int Np = h->Np, Ny = h->Ny, d = h->d, Bp = round_up(n, 64);
    DevArena mem;                   // device scratch of this call; released on every way out, before the append allocates
    double* VT = mem.take<double>((size_t)Ny * Bp * Np);
    double* S = mem.take<double>((size_t)Ny * Bp * Bp);
    double* GT = mem.take<double>((size_t)Ny * k * Bp);
    double* dg = mem.take<double>((size_t)2 * Ny * Bp);
    double* score = mem.take<double>((size_t)2 * Bp);
    double* dgain = mem.take<double>((size_t)k);
    int* dsel = mem.take<int>((size_t)k);
    int* flags = mem.take<int>((size_t)(k + 2));
    HIPCHK(mem.status);
    HIPCHK(hipMemsetAsync(flags, 0, (size_t)(k + 2) * sizeof(int), cx.stream));
    HIPCHK(hipMemcpyAsync(h->Z, Xcand, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, cx.stream));
    // S_a = k_a(C, C) - V^T V on the route of gpmpc_covar (api_predict.inl), without its refinement step
    launch_crosscov(cx.stream, d, h->XT, h->ws.hyper, h->ws.alpha, h->Z, h->KsT, h->meanT, nullptr, h->N, Np, n, Bp, Ny);
    launch_vt(cx, h->KsT, h->ws.Inv, VT, Bp, Np, Ny);
    launch_neg_gram(cx, VT, S, Bp, Np, Ny);
    hipLaunchKernelGGL(select_schur_kernel, dim3((Bp + 255) / 256, Bp, Ny), dim3(256), 0, cx.stream, h->Z, h->ws.hyper, S, n, Bp, d);
    hipLaunchKernelGGL(select_init_kernel, dim3((Bp + 255) / 256), dim3(256), 0, cx.stream, S, dg, score, n, Bp, Ny);
    for (int t = 0; t < k; ++t)
        hipLaunchKernelGGL(select_step_kernel, dim3(Bp / 64), dim3(256), 0, cx.stream, S, GT, dg, score, h->ws.hyper,
                           h->ws.jitter, dsel, dgain, flags, n, Bp, k, Ny, d, t, min_gain);
    HIPCHK(hipGetLastError());
    picks.assign(k, -1);
    gains.assign(k, 0.0);
    kout = 0;
    HIPCHK(hipMemcpyAsync(picks.data(), dsel, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, cx.stream));
    HIPCHK(hipMemcpyAsync(gains.data(), dgain, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, cx.stream));
    HIPCHK(hipMemcpyAsync(&kout, flags, sizeof(int), hipMemcpyDeviceToHost, cx.stream));
    HIPCHK(hipStreamSynchronize(cx.stream));
    if (kout < 0 || kout > k) return fail(GPMPC_EHIP, "append_select: the device reported %d picks of %d", kout, k);
    for (int t = 0; t < kout; ++t)
        if (picks[t] < 0 || picks[t] >= n) return fail(GPMPC_EHIP, "append_select: pick %d is candidate %d of %d", t, picks[t], n);
    return GPMPC_OK;
}

extern "C" int gpmpc_append_select(gpmpc_gp* h, int n, const double* Xcand, const double* Ycand, int k, double min_gain,
                                   int* selected, double* gain, int* k_out, int* info) {
    if (!h || !Xcand || !selected) return fail(GPMPC_EINVAL, "NULL handle, candidates or selected");
    CHK(refuse_sparse(h, "gpmpc_append_select"));
    if (n <= 0 || k < 1 || k > n) return fail(GPMPC_EINVAL, "append_select: need 1 <= k <= n (k = %d, n = %d)", k, n);
    if (!(min_gain == min_gain)) return fail(GPMPC_EINVAL, "append_select: min_gain is NaN");
    if (!h->fitted) return fail(GPMPC_ENOTFIT, "model has no factors (call gpmpc_fit or gpmpc_set_factors)");
    if (n > chunk_size(h)) return fail(GPMPC_EINVAL, "append_select: n=%d exceeds the single-chunk limit %d", n, chunk_size(h));
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> picks;
    std::vector<double> gains;
    int kout = 0;
    const int rc = select_greedy(h, n, Xcand, k, min_gain, picks, gains, kout);
    if (rc != GPMPC_OK) {
        hipStreamSynchronize(h->stream);
        return rc;
    }
    for (int t = 0; t < kout; ++t) {
        selected[t] = picks[t];
        if (gain) gain[t] = gains[t];
    }
    if (k_out) *k_out = kout;
    if (info) std::fill(info, info + h->Ny, 0);
    if (!Ycand || kout == 0) return GPMPC_OK;             // selection only / nothing worth a pick: the model is untouched
    const int d = h->d, Ny = h->Ny;
    std::vector<double> Xs((size_t)kout * d), Ys((size_t)kout * Ny);
    for (int t = 0; t < kout; ++t) {
        std::memcpy(&Xs[(size_t)t * d], Xcand + (size_t)picks[t] * d, d * sizeof(double));
        std::memcpy(&Ys[(size_t)t * Ny], Ycand + (size_t)picks[t] * Ny, Ny * sizeof(double));
    }
    return gpmpc_append(h, kout, Xs.data(), Ys.data(), info);
}
