// api_select.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: gpmpc_append_select -- greedy max-variance choice among candidate points (select_kernels.hpp), then gpmpc_append
// of the chosen rows.
// ------------------------------------------------------------------------------------------------
namespace {
struct SelectScratch {              // device scratch of one call; released on every way out, before the append allocates
    double *VT = nullptr, *S = nullptr, *GT = nullptr, *dg = nullptr, *score = nullptr, *gain = nullptr;
    int *sel = nullptr, *flags = nullptr;
    ~SelectScratch() {
        hipFree(VT); hipFree(S); hipFree(GT); hipFree(dg); hipFree(score); hipFree(gain); hipFree(sel); hipFree(flags);
    }
};
}  // namespace

// The selection alone: picks[0 .. kout), gains[0 .. kout).  Everything n x n stays on the device.
static int select_greedy(gpmpc_gp* h, int n, const double* Xcand, int k, double min_gain, std::vector<int>& picks,
                         std::vector<double>& gains, int& kout) {
    CHK(ensure_scratch(h, n));
    const Ctx cx = h->cx();
    const int Np = h->Np, Ny = h->Ny, d = h->d, Bp = round_up(n, 64);
    SelectScratch s;
    HIPCHK(hipMalloc(&s.VT, (size_t)Ny * Bp * Np * sizeof(double)));
    HIPCHK(hipMalloc(&s.S, (size_t)Ny * Bp * Bp * sizeof(double)));
    HIPCHK(hipMalloc(&s.GT, (size_t)Ny * k * Bp * sizeof(double)));
    HIPCHK(hipMalloc(&s.dg, (size_t)2 * Ny * Bp * sizeof(double)));
    HIPCHK(hipMalloc(&s.score, (size_t)2 * Bp * sizeof(double)));
    HIPCHK(hipMalloc(&s.gain, (size_t)k * sizeof(double)));
    HIPCHK(hipMalloc(&s.sel, (size_t)k * sizeof(int)));
    HIPCHK(hipMalloc(&s.flags, (size_t)(k + 2) * sizeof(int)));
    // (plain pointers for the launches: a launch argument list must not hold the owning struct itself)
    double *VT = s.VT, *S = s.S, *GT = s.GT, *dg = s.dg, *score = s.score, *dgain = s.gain;
    int *dsel = s.sel, *flags = s.flags;
    HIPCHK(hipMemsetAsync(flags, 0, (size_t)(k + 2) * sizeof(int), cx.stream));
    HIPCHK(hipMemcpyAsync(h->Z, Xcand, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, cx.stream));
    // S_a = k_a(C, C) - V^T V on the route of gpmpc_covar (api_predict.inl)
    launch_crosscov(cx.stream, d, h->XT, h->ws.hyper, h->ws.alpha, h->Z, h->KsT, h->meanT, nullptr, h->N, Np, n, Bp, Ny);
    GemmP p = gemm_base(cx);  // VT[j][i] = sum_k KsT[j][k] invL[i][k]
    p.A = h->KsT; p.lda = Np; p.sA = (long)Bp * Np; p.a_mc = 0;
    p.B = h->ws.Inv; p.ldb = Np; p.sB = (long)Np * Np; p.b_nc = 0; p.kflags = KB_LE_N;
    p.C = VT; p.ldc = Np; p.sC = (long)Bp * Np;
    p.M = Bp; p.N = Np; p.K = Np;
    launch_gemm(p, Ny, cx.stream);
    GemmP q = gemm_base(cx);  // S = -VT VT^T
    q.A = VT; q.lda = Np; q.sA = (long)Bp * Np; q.a_mc = 0;
    q.B = VT; q.ldb = Np; q.sB = (long)Bp * Np; q.b_nc = 0;
    q.C = S; q.ldc = Bp; q.sC = (long)Bp * Bp;
    q.M = Bp; q.N = Bp; q.K = Np; q.alpha = -1.0;
    launch_gemm(q, Ny, cx.stream);
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
