// api_sparse.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: gpmpc_sparse_fitc -- a FITC model on M inducing points as an ordinary handle of size M (fitc_kernels.hpp).
//
// With Sigma = Kuu + Kuf Lambda^-1 Kfu and P = Kuu^-1 - Sigma^-1 the FITC predictor is mean = k(z, Xu) alpha_u,
// var = sf^2 - k(z, Xu) P k(Xu, z): an exact GP's formulas on the inducing points with K^-1 -> P, and the exact-moment sums
// hold with the same substitution.  Every entry point of this library evaluates those formulas from (X, L, L^-1, alpha,
// K^-1) of a handle, so the build ends in a LOWER triangular W with W^T W = P and hands out a handle with L^-1 = W,
// L = W^-1, K^-1 = P, alpha = alpha_u and the targets Yu = L L^T alpha_u that make alpha = K^-1 y hold for it.
//   Luu = chol(Kuu + 1e-6 sf^2 I)      a fit of the new handle on (Xu, 0) with the jitter in place of the noise
//   B = I + Vs Vs^T, r = Vs ys         chunk loop over the training points (two O(N M^2) products per chunk)
//   alpha_u = Luu^-T B^-1 r,   C = I - B^-1,   P = Luu^-T C Luu^-1, then (P + P^T) / 2
//   W = S Luu^-1 with C = S^T S, S lower triangular (the Cholesky factor of the index-reversed C, transposed and reversed back):
//   the same W as from the reversed Cholesky of P, which is unique.
// Nothing of size N x N is allocated and nothing N-sized goes to the host.
// ------------------------------------------------------------------------------------------------
namespace {
struct FitcScratch {                // device scratch of one build and the handle under construction; released on every way out
    DevArena mem;                   // VT, ys, Bm, r, hyp of fitc_build
    Workspace tw;                   // M-sized workspace of the two factorisations (B, the reversed P)
    gpmpc_gp* s = nullptr;
    ~FitcScratch() {
        ws_free(tw);
        if (s) {
            const std::string keep = g_err;
            gpmpc_destroy(s);
            g_err = keep;
        }
    }
};
}  // namespace

// status words of a factor_blocked on `ws` -> info[a] = -(first bad pivot); true if any
static int fitc_check_pd(gpmpc_gp* s, Workspace& ws, int* info, const char* what) {
    std::vector<int> inf(ws.batch, 0);
    HIPCHK(hipMemcpyAsync(inf.data(), ws.info, ws.batch * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    bool bad = false;
    for (int a = 0; a < ws.batch; ++a)
        if (inf[a] != 0) {
            bad = true;
            if (info) info[a] = -inf[a];
        }
    if (bad) return fail(GPMPC_ENOTPD, "sparse_fitc: %s is not positive definite", what);
    return GPMPC_OK;
}

static int fitc_build(gpmpc_gp* h, gpmpc_gp* s, FitcScratch& sc, const std::vector<double>& hy, int* info) {
    const int N = h->N, NpS = h->Np, d = h->d, Ny = h->Ny, M = s->N, Mp = s->Np;
    const long sM = (long)Mp * Mp;
    // Luu and Luu^-1: the new handle's own fit on (Xu, 0), noise (1e-3 sf)^2 = GPML's inducing jitter
    std::vector<double> hj = hy;
    for (int a = 0; a < Ny; ++a) hj[(size_t)a * (d + 2) + d + 1] = 1e-3 * hy[(size_t)a * (d + 2) + d];
    CHK(fit_impl(s, hj.data(), 0, info, nullptr));
    alpha_ready(s);
    const int chunk = chunk_size(s);
    CHK(ensure_scratch(s, std::min(N, chunk)));
    const int Bcp = round_up(std::min(N, chunk), 64);
    const Ctx cx = s->cx();
    double* VT = sc.mem.take<double>((size_t)Ny * Bcp * Mp);
    double* ys = sc.mem.take<double>((size_t)Ny * Bcp);
    double* Bm = sc.mem.take<double>((size_t)Ny * sM);
    double* r = sc.mem.take<double>((size_t)Ny * Mp);
    double* hyp = sc.mem.take<double>((size_t)Ny * (d + 2));
    HIPCHK(sc.mem.status);
    CHK(ws_alloc(sc.tw, Ny, Mp, d));
    Workspace& tw = sc.tw;
    HIPCHK(hipMemcpyAsync(hyp, hy.data(), (size_t)Ny * (d + 2) * sizeof(double), hipMemcpyHostToDevice, cx.stream));
    HIPCHK(hipMemsetAsync(r, 0, (size_t)Ny * Mp * sizeof(double), cx.stream));
    hipLaunchKernelGGL(fitc_eye_kernel, dim3((unsigned)(sM / 256), Ny), dim3(256), 0, cx.stream, Bm, Mp);
    const int T = Mp / 64;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int nc = std::min(chunk, N - c0), Bp = round_up(nc, 64);
        hipLaunchKernelGGL(fitc_gather_kernel, dim3((nc * d + 255) / 256), dim3(256), 0, cx.stream, (const double*)h->XT, s->Z, NpS,
                           c0, nc, d);
        launch_crosscov(cx.stream, d, s->XT, s->ws.hyper, s->ws.alpha, s->Z, s->KsT, s->meanT, nullptr, M, Mp, nc, Bp, Ny);
        launch_vt(cx, s->KsT, s->ws.Inv, VT, Bp, Mp, Ny);   // VT[c][m] = sum_k KsT[c][k] Luu^-1[m][k]
        hipLaunchKernelGGL(fitc_scale_kernel, dim3(Bp / 4, Ny), dim3(256), 0, cx.stream, VT, (const double*)h->Y, (const double*)hyp,
                           ys, c0, nc, Bp, M, Mp, NpS, d);
        PhaseTimer t(s, GPMPC_PH_VARGEMM);                  // (profiling follows the source handle: gpmpc_sparse_fitc below)
        hipLaunchKernelGGL(fitc_syrk_kernel, dim3(T * (T + 1) / 2, Ny), dim3(256), 0, cx.stream, (const double*)VT,
                           (const double*)ys, Bm, r, Bp, Mp, cx.crow_mode);
    }
    hipLaunchKernelGGL(symmetrize_kernel, dim3(T, T, Ny), dim3(256), 0, cx.stream, Bm, Mp);
    HIPCHK(hipGetLastError());
    // ---- the M x M tail ----
    HIPCHK(hipMemcpyAsync(tw.K, Bm, (size_t)Ny * sM * sizeof(double), hipMemcpyDeviceToDevice, cx.stream));
    factor_blocked(cx, tw, true);                           // LB = chol(B), LB^-1
    CHK(fitc_check_pd(s, tw, info, "B = I + Vs Vs^T"));
    solve_alpha(cx, tw, r, Mp);                             // tw.alpha = B^-1 r
    HIPCHK(hipMemcpyAsync(s->ws.w, tw.alpha, (size_t)Ny * Mp * sizeof(double), hipMemcpyDeviceToDevice, cx.stream));
    solve_alpha_from_w(cx, s->ws, Ny, nullptr);             // alpha_u = Luu^-T B^-1 r
    CHK(compute_invK(cx, tw));                              // B^-1 (lower triangle by MFMA, mirrored)
    hipLaunchKernelGGL(fitc_cmat_kernel, dim3((unsigned)(sM / 256), Ny), dim3(256), 0, cx.stream, tw.InvK, M, Mp);
    GemmP g = gemm_base(cx);                                // G = C Luu^-1
    g.A = tw.InvK; g.lda = Mp; g.sA = sM; g.a_mc = 0;
    g.B = s->ws.Inv; g.ldb = Mp; g.sB = sM; g.b_nc = 1; g.kflags = KB_GE_N;
    g.C = Bm; g.ldc = Mp; g.sC = sM;
    g.M = Mp; g.N = Mp; g.K = Mp;
    launch_gemm(g, Ny, cx.stream);
    CHK(ws_need_invK(s->ws));
    GemmP q = gemm_base(cx);                                // P = Luu^-T G, both triangles; their average is symmetric to the bit
    q.A = s->ws.Inv; q.lda = Mp; q.sA = sM; q.a_mc = 1;
    q.B = Bm; q.ldb = Mp; q.sB = sM; q.b_nc = 1;
    q.C = s->ws.InvK; q.ldc = Mp; q.sC = sM;
    q.M = Mp; q.N = Mp; q.K = Mp;
    launch_gemm(q, Ny, cx.stream);
    hipLaunchKernelGGL(fitc_symavg_kernel, dim3(T, T, Ny), dim3(256), 0, cx.stream, s->ws.InvK, Mp);
    // W: lower triangular with W^T W = P.  With C = S^T S, S lower triangular -- the Cholesky factor of the index-reversed C,
    // transposed and reversed back -- W = S Luu^-1 is a product of two lower triangular matrices and W^-1 = Luu S^-1.  That is
    // the factor the reversed Cholesky of P itself gives (it is unique), from a matrix with eigenvalues in [0, 1) instead of one
    // with entries ~ 1 / jitter.  C is singular where no training point bears on an inducing direction (two equal inducing
    // points: exactly): if a pivot comes out non-positive the factorisation is repeated ONCE on C + shift I, shift = 8 Mp eps
    // -- W^T W = P + shift Kuu^-1 then, a variance too small by shift |Luu^-1 k|^2 <= shift sf^2; K^-1 = P stays as it is.
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double shift = attempt ? 8.0 * Mp * 2.220446049250313e-16 : 0.0;
        hipLaunchKernelGGL(fitc_revt_kernel, dim3(T, T, Ny), dim3(256), 0, cx.stream, (const double*)tw.InvK, tw.K, Mp, 1, shift, M);
        HIPCHK(hipMemsetAsync(tw.info, 0, Ny * sizeof(int), cx.stream));
        factor_blocked(cx, tw, true);                       // Lr = chol(reversed C), Lr^-1
        std::vector<int> inf(Ny, 0);
        const int rc = fitc_check_pd(s, tw, attempt ? info : inf.data(), "C = I - B^-1 (reversed Cholesky)");
        if (rc == GPMPC_OK) break;
        if (attempt) return rc;
    }
    // S = J Lr^T J -> tw.K, S^-1 = J Lr^-T J -> Bm (both free by now); the padding stays the identity
    hipLaunchKernelGGL(fitc_revt_kernel, dim3(T, T, Ny), dim3(256), 0, cx.stream, (const double*)tw.L, tw.K, Mp, 1, 0.0, M);
    hipLaunchKernelGGL(fitc_revt_kernel, dim3(T, T, Ny), dim3(256), 0, cx.stream, (const double*)tw.Inv, Bm, Mp, 1, 0.0, M);
    GemmP wq = gemm_base(cx);                               // W = S Luu^-1 -> tw.L
    wq.A = tw.K; wq.lda = Mp; wq.sA = sM; wq.a_mc = 0; wq.kflags = KA_LE_M;
    wq.B = s->ws.Inv; wq.ldb = Mp; wq.sB = sM; wq.b_nc = 1;
    wq.C = tw.L; wq.ldc = Mp; wq.sC = sM;
    wq.M = Mp; wq.N = Mp; wq.K = Mp;
    launch_gemm(wq, Ny, cx.stream);
    GemmP lq = gemm_base(cx);                               // W^-1 = Luu S^-1 -> tw.Inv
    lq.A = s->ws.L; lq.lda = Mp; lq.sA = sM; lq.a_mc = 0; lq.kflags = KA_LE_M;
    lq.B = Bm; lq.ldb = Mp; lq.sB = sM; lq.b_nc = 1;
    lq.C = tw.Inv; lq.ldc = Mp; lq.sC = sM;
    lq.M = Mp; lq.N = Mp; lq.K = Mp;
    launch_gemm(lq, Ny, cx.stream);
    // the handle's L^-1 = W and L = W^-1 (Luu and Luu^-1 have served)
    HIPCHK(hipMemcpyAsync(s->ws.Inv, tw.L, (size_t)Ny * sM * sizeof(double), hipMemcpyDeviceToDevice, cx.stream));
    HIPCHK(hipMemcpyAsync(s->ws.L, tw.Inv, (size_t)Ny * sM * sizeof(double), hipMemcpyDeviceToDevice, cx.stream));
    // w = L^T alpha_u (what the fused-mean variance product reads), Yu = L w
    const int chunks = (Mp + GEMVT_ROWS - 1) / GEMVT_ROWS;
    hipLaunchKernelGGL(gemv_lowerT_part_kernel, dim3((Mp + 127) / 128, chunks, Ny), dim3(256), 0, cx.stream, (const double*)s->ws.L,
                       (const double*)s->ws.alpha, s->ws.W, Mp, sM, (long)Mp, s->ws.wstride(), (const int*)nullptr);
    hipLaunchKernelGGL(gemv_lowerT_finish_kernel, dim3((Mp + 255) / 256, Ny), dim3(256), 0, cx.stream, (const double*)s->ws.W, s->ws.w,
                       Mp, chunks, s->ws.wstride(), (long)Mp, (const int*)nullptr);
    hipLaunchKernelGGL(gemv_rows_kernel, dim3(Mp / 4, Ny), dim3(256), 0, cx.stream, (const double*)s->ws.L, (const double*)s->ws.w,
                       s->Y, Mp, sM, (long)Mp, (long)Mp, 1);
    HIPCHK(hipMemcpyAsync(s->ws.hyper, hyp, (size_t)Ny * (d + 2) * sizeof(double), hipMemcpyDeviceToDevice, cx.stream));
    HIPCHK(hipMemsetAsync(s->ws.jitter, 0, Ny * sizeof(double), cx.stream));
    HIPCHK(hipStreamSynchronize(cx.stream));
    HIPCHK(hipGetLastError());
    s->hyper = hy;
    s->fitted = true;
    s->have_invK = true;
    s->have_beta = false;
    s->tail.armed = false;
    s->nll_last_a = -1;
    s->sparse = true;
    return GPMPC_OK;
}

extern "C" int gpmpc_sparse_fitc(gpmpc_gp* h, const double* hyper, int M, const double* Xu, int* info, gpmpc_gp** out) {
    if (!out) return fail(GPMPC_EINVAL, "sparse_fitc: out is NULL");
    *out = nullptr;
    if (!h || !Xu) return fail(GPMPC_EINVAL, "sparse_fitc: NULL handle or inducing points");
    if (M < 1 || M > h->N) return fail(GPMPC_EINVAL, "sparse_fitc: need 1 <= M <= N (M = %d, N = %d)", M, h->N);
    if (h->mean_kind != GPMPC_MEAN_ZERO) return fail(GPMPC_EINVAL, "sparse_fitc: the source model must have the zero prior mean");
    if (h->sparse) return fail(GPMPC_EINVAL, "sparse_fitc: the source is itself a FITC sparse model");
    if (!hyper && !h->fitted) return fail(GPMPC_ENOTFIT, "sparse_fitc: hyper is NULL and the source model has no factors");
    const int d = h->d, Ny = h->Ny;
    const double* src = hyper ? hyper : h->hyper.data();
    const std::vector<double> hy(src, src + (size_t)Ny * (d + 2));
    for (int a = 0; a < Ny; ++a)
        for (int k = 0; k < d + 2; ++k) {
            const double v = hy[(size_t)a * (d + 2) + k];
            if (!std::isfinite(v) || (k <= d && v == 0.0))
                return fail(GPMPC_EINVAL, "hyper[%d][%d] = %g is not a usable SE-ARD parameter", a, k, v);
        }
    for (size_t i = 0; i < (size_t)M * d; ++i)
        if (!std::isfinite(Xu[i])) return fail(GPMPC_EINVAL, "sparse_fitc: Xu[%zu] is not finite", i);
    HIPCHK(hipSetDevice(h->device));
    alpha_ready(h);
    HIPCHK(hipStreamSynchronize(h->stream));                // the source's data are read on the new handle's queue
    if (info) std::fill(info, info + Ny, 0);
    FitcScratch sc;
    {
        const std::vector<double> y0((size_t)M * Ny, 0.0);
        CHK(gpmpc_create(h->device, M, d, Ny, Xu, y0.data(), &sc.s));
    }
    sc.s->prof.on = h->prof.on;                             // the build is bracketed like the source's own calls; the rank
    sc.s->prof.mask = h->prof.mask;                         // updates B += Vs Vs^T go under GPMPC_PH_VARGEMM of the NEW handle
    const int rc = fitc_build(h, sc.s, sc, hy, info);
    if (rc != GPMPC_OK) {
        if (sc.s) hipStreamSynchronize(sc.s->stream);
        return rc;                                          // (the scratch's destructor releases the half-built handle)
    }
    *out = sc.s;
    sc.s = nullptr;
    return GPMPC_OK;
}
