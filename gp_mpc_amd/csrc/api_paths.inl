// api_paths.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: pathwise posterior samples (paths_kernels.hpp): draw S functions once, evaluate them per particle or on a grid,
// and the consistent Monte Carlo roll-out gpmpc_rollout_paths.

constexpr int PATHS_SETUP_COLS = 512;   // path columns per pass of the setup (its two Np x cols scratch panels per output)

static int paths_grow(double** p, size_t* cap, size_t need) {
    if (need <= *cap) return GPMPC_OK;
    hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc(p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return fail(GPMPC_ENOMEM, "pathwise samples: no device memory for %zu MB", need * sizeof(double) >> 20);
    }
    *cap = need;
    return GPMPC_OK;
}

// the [inputs | scratch | results] device block of gpmpc_paths_eval / gpmpc_rollout_paths and its pinned mirror (grow-only)
static int paths_io_reserve(gpmpc_gp* h, size_t dev_doubles, size_t pin_doubles) {
    if (dev_doubles <= h->pio_cap && pin_doubles <= h->pio_pin_cap) return GPMPC_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(h->pio_dev);
    if (h->pio_pin) hipHostFree(h->pio_pin);
    h->pio_dev = h->pio_pin = nullptr;
    const size_t cap = std::max(h->pio_cap, dev_doubles), pin_cap = std::max(h->pio_pin_cap, pin_doubles);
    h->pio_cap = h->pio_pin_cap = 0;
    HIPCHK(hipMalloc(&h->pio_dev, cap * sizeof(double)));
    HIPCHK(hipHostMalloc((void**)&h->pio_pin, pin_cap * sizeof(double), hipHostMallocDefault));
    h->pio_cap = cap;
    h->pio_pin_cap = pin_cap;
    return GPMPC_OK;
}

// a handle with factors and valid paths, or the error to return
static int paths_ready(gpmpc_gp* h, const char* what) {
    if (!h) return fail(GPMPC_EINVAL, "NULL handle");
    if (!h->fitted) return fail(GPMPC_ENOTFIT, "model has no factors (call gpmpc_fit or gpmpc_set_factors)");
    if (h->pS <= 0 || h->p_gen < 0) return fail(GPMPC_EINVAL, "%s: no paths drawn (call gpmpc_paths_draw)", what);
    if (h->p_gen != h->factor_gen)
        return fail(GPMPC_EINVAL, "%s: the paths are stale, the factors or the data changed since gpmpc_paths_draw; draw again", what);
    return GPMPC_OK;
}

static int paths_part_reserve(gpmpc_gp* h) {
    const size_t need = (size_t)paths_part_blocks(h->N, h->pF) * h->Ny * h->pSld;
    if (need <= h->pPart_cap) return GPMPC_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    return paths_grow(&h->pPart, &h->pPart_cap, need);
}

extern "C" int gpmpc_paths_free(gpmpc_gp* h) {
    if (!h) return fail(GPMPC_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (double** p : {&h->pV, &h->pWT, &h->pOmega, &h->pPart}) {
        hipFree(*p);
        *p = nullptr;
    }
    h->pV_cap = h->pWT_cap = h->pOmega_cap = h->pPart_cap = 0;
    hipFree(h->pio_dev);
    if (h->pio_pin) hipHostFree(h->pio_pin);
    h->pio_dev = h->pio_pin = nullptr;
    h->pio_cap = h->pio_pin_cap = 0;
    h->pS = h->pSld = h->pF = h->pFp = 0;
    h->p_gen = -1;
    return GPMPC_OK;
}

extern "C" int gpmpc_paths_draw(gpmpc_gp* h, int S, int F, unsigned long long seed, const double* eps_omega, const double* w,
                                const double* xi) {
    if (!h) return fail(GPMPC_EINVAL, "NULL handle");
    if (!h->fitted) return fail(GPMPC_ENOTFIT, "model has no factors (call gpmpc_fit or gpmpc_set_factors)");
    if (h->sparse)
        return fail(GPMPC_EINVAL, "gpmpc_paths_draw: this handle is a FITC sparse model; a sample of its predictor is another construction");
    if (S < 1 || S > (1 << 20)) return fail(GPMPC_EINVAL, "bad S = %d (1 .. 2^20 paths)", S);
    if (F < 2 || F > 65536 || (F & 1)) return fail(GPMPC_EINVAL, "bad F = %d (an even number of features, 2 .. 65536)", F);
    HIPCHK(hipSetDevice(h->device));
    h->tail.armed = false;
    alpha_ready(h);
    const int Ny = h->Ny, d = h->d, N = h->N, Np = h->Np, F2 = F / 2;
    const int Sld = (S + 1) & ~1, Fp = round_up(F, 16);
    const int cols = std::min(Sld, PATHS_SETUP_COLS);
    const long ldr = cols;
    const size_t nV = (size_t)Ny * Np * Sld, nW = (size_t)Ny * Fp * Sld + Sld, nO = (size_t)Ny * F2 * d;
    // (nW: one row of slack -- the DMA-staged product clamps the columns of a column panel of WT to the row length, not to the panel)
    HIPCHK(hipStreamSynchronize(h->stream));
    // the call's scratch first: while nothing of the earlier paths has been touched a failed allocation leaves them valid
    DevArena mem;
    double* Phi = mem.take<double>((size_t)Ny * Np * Fp);
    double* R = mem.take<double>((size_t)Ny * Np * ldr);
    double* T1 = mem.take<double>((size_t)Ny * Np * ldr);
    double* dEo = eps_omega ? mem.take<double>(nO) : nullptr;
    double* dW = w ? mem.take<double>((size_t)Ny * S * F) : nullptr;
    double* dXi = xi ? mem.take<double>((size_t)Ny * S * N) : nullptr;
    if (mem.status != hipSuccess) {
        (void)hipGetLastError();
        return fail(GPMPC_ENOMEM, "pathwise samples: no device memory for the setup's scratch");
    }
    if (nV > h->pV_cap || nW > h->pWT_cap || nO > h->pOmega_cap) h->p_gen = -1;     // a buffer is replaced: the earlier paths go
    CHK(paths_grow(&h->pV, &h->pV_cap, nV));
    CHK(paths_grow(&h->pWT, &h->pWT_cap, nW));
    CHK(paths_grow(&h->pOmega, &h->pOmega_cap, nO));
    h->p_gen = -1;                                  // the buffers are about to be overwritten
    hipStream_t st = h->stream;
    if (dEo) HIPCHK(hipMemcpyAsync(dEo, eps_omega, nO * sizeof(double), hipMemcpyHostToDevice, st));
    if (dW) HIPCHK(hipMemcpyAsync(dW, w, (size_t)Ny * S * F * sizeof(double), hipMemcpyHostToDevice, st));
    if (dXi) HIPCHK(hipMemcpyAsync(dXi, xi, (size_t)Ny * S * N * sizeof(double), hipMemcpyHostToDevice, st));
    const Ctx cx = h->cx();
    auto blocks = [](size_t items) { return dim3((unsigned)((items + 255) / 256)); };
    {
        ProfScope t(&h->prof, st, GPMPC_PH_MC);
        HIPCHK(hipMemsetAsync(h->pWT, 0, nW * sizeof(double), st));
        hipLaunchKernelGGL(paths_omega_kernel, blocks((size_t)Ny * F2 * ((d + 1) / 2)), dim3(256), 0, st, h->ws.hyper, dEo, seed,
                           h->pOmega, Ny, F2, d);
        hipLaunchKernelGGL(paths_wt_kernel, blocks((size_t)Ny * (Fp / 2) * Sld), dim3(256), 0, st, dW, seed, h->pWT, Ny, S, Sld, F, Fp);
        hipLaunchKernelGGL(paths_phi_kernel, blocks((size_t)Ny * Np * (Fp / 2)), dim3(256), 0, st, h->XT, 1L, (long)Np, h->pOmega,
                           h->ws.hyper, Phi, Ny, N, Np, F, Fp, d);
        for (int c0 = 0; c0 < Sld; c0 += cols) {
            const int nc = std::min(cols, Sld - c0);
            hipLaunchKernelGGL(paths_xi_kernel, blocks((size_t)Ny * (Np / 2) * nc), dim3(256), 0, st, dXi, seed, h->ws.hyper, R, ldr,
                               (long)Np * ldr, Ny, N, Np, S, c0, nc, d);
            GemmP r = gemm_base(cx);                    // R = Phi W^T + sn xi
            r.A = Phi; r.lda = Fp; r.sA = (long)Np * Fp; r.a_mc = 0;
            r.B = h->pWT + c0; r.ldb = Sld; r.sB = (long)Fp * Sld; r.b_nc = 1;
            r.C = R; r.ldc = ldr; r.sC = (long)Np * ldr;
            r.M = Np; r.N = nc; r.K = Fp; r.beta = 1.0;
            launch_gemm(r, Ny, st);
            GemmP t1 = gemm_base(cx);                   // T1 = L^-1 R
            t1.A = h->ws.Inv; t1.lda = Np; t1.sA = h->ws.mat(); t1.a_mc = 0; t1.kflags = KA_LE_M;
            t1.B = R; t1.ldb = ldr; t1.sB = (long)Np * ldr; t1.b_nc = 1;
            t1.C = T1; t1.ldc = ldr; t1.sC = (long)Np * ldr;
            t1.M = Np; t1.N = nc; t1.K = Np;
            launch_gemm(t1, Ny, st);
            hipLaunchKernelGGL(paths_alpha_fill_kernel, blocks((size_t)Ny * Np * nc), dim3(256), 0, st, h->ws.alpha, h->pV, (long)Sld,
                               Ny, Np, c0, nc);
            GemmP u = gemm_base(cx);                    // V = alpha - L^-T T1
            u.A = h->ws.Inv; u.lda = Np; u.sA = h->ws.mat(); u.a_mc = 1; u.kflags = KA_GE_M;
            u.B = T1; u.ldb = ldr; u.sB = (long)Np * ldr; u.b_nc = 1;
            u.C = h->pV + c0; u.ldc = Sld; u.sC = (long)Np * Sld;
            u.M = Np; u.N = nc; u.K = Np; u.alpha = -1.0; u.beta = 1.0;
            launch_gemm(u, Ny, st);
        }
    }
    hipError_t e = hipStreamSynchronize(st);            // (the scratch goes when `mem` does)
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GPMPC_EHIP, "%s", hipGetErrorString(e));
    h->pS = S; h->pSld = Sld; h->pF = F; h->pFp = Fp;
    h->p_gen = h->factor_gen;
    return GPMPC_OK;
}

extern "C" int gpmpc_paths_get(gpmpc_gp* h, int* S, int* F, double* omega, double* w, double* v) {
    CHK(paths_ready(h, "gpmpc_paths_get"));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int Ny = h->Ny, N = h->N, Np = h->Np, pS = h->pS, Sld = h->pSld, pF = h->pF, Fp = h->pFp;
    if (S) *S = pS;
    if (F) *F = pF;
    if (omega) HIPCHK(hipMemcpy(omega, h->pOmega, (size_t)Ny * (pF / 2) * h->d * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> tmp;
    for (int a = 0; a < Ny && (w || v); ++a) {          // the device layouts have the paths contiguous: transposed on the host
        if (w) {
            tmp.resize((size_t)Fp * Sld);
            HIPCHK(hipMemcpy(tmp.data(), h->pWT + (size_t)a * Fp * Sld, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int s = 0; s < pS; ++s)
                for (int j = 0; j < pF; ++j) w[((size_t)a * pS + s) * pF + j] = tmp[(size_t)j * Sld + s];
        }
        if (v) {
            tmp.resize((size_t)Np * Sld);
            HIPCHK(hipMemcpy(tmp.data(), h->pV + (size_t)a * Np * Sld, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int s = 0; s < pS; ++s)
                for (int i = 0; i < N; ++i) v[((size_t)a * pS + s) * N + i] = tmp[(size_t)i * Sld + s];
        }
    }
    return GPMPC_OK;
}

// partial sums of every path at its input dZ[S][d] -> h->pPart (paths_finish_kernel adds them)
static void paths_eval_launch(gpmpc_gp* h, const double* dZ) {
    launch_paths_eval(h->stream, h->d, h->XT, h->ws.hyper, h->pV, h->pWT, h->pOmega, dZ, h->pPart, h->N, h->Np, h->pS, h->pSld,
                      h->pF, h->pFp, h->Ny);
}

extern "C" int gpmpc_paths_eval(gpmpc_gp* h, const double* Z, double* f) {
    CHK(paths_ready(h, "gpmpc_paths_eval"));
    if (!Z || !f) return fail(GPMPC_EINVAL, "NULL Z or f");
    HIPCHK(hipSetDevice(h->device));
    const int S = h->pS, d = h->d, Ny = h->Ny;
    const size_t nZ = (size_t)S * d, nF = (size_t)S * Ny;
    CHK(paths_part_reserve(h));
    CHK(paths_io_reserve(h, nZ + nF, nZ + nF));
    std::memcpy(h->pio_pin, Z, nZ * sizeof(double));
    HIPCHK(hipMemcpyAsync(h->pio_dev, h->pio_pin, nZ * sizeof(double), hipMemcpyHostToDevice, h->stream));
    double *dZ = h->pio_dev, *dF = h->pio_dev + nZ;
    {                                                   // (the hot kernel alone under GPMPC_PH_MC: tools/paths_rollout_times.py)
        ProfScope t(&h->prof, h->stream, GPMPC_PH_MC);
        paths_eval_launch(h, dZ);
    }
    {
        ProfScope t(&h->prof, h->stream, GPMPC_PH_FINISH);
        const bool madd = h->mean_kind && h->mean_add;
        hipLaunchKernelGGL(paths_finish_kernel, dim3((unsigned)((S + MC_BLOCK - 1) / MC_BLOCK)), dim3(MC_BLOCK), 0, h->stream, h->pPart,
                           paths_part_blocks(h->N, h->pF), dZ, h->mpar, madd ? h->mean_kind : 0, h->ws.hyper, 0, (const double*)nullptr,
                           0ull, 0u, dF, (double*)nullptr, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                           (const double*)nullptr, (const double*)nullptr, S, h->pSld, Ny, d);
    }
    hipError_t e = hipMemcpyAsync(h->pio_pin + nZ, dF, nF * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GPMPC_EHIP, "%s", hipGetErrorString(e));
    std::memcpy(f, h->pio_pin + nZ, nF * sizeof(double));
    return GPMPC_OK;
}

extern "C" int gpmpc_paths_eval_grid(gpmpc_gp* h, int B, const double* Z, double* f) {
    CHK(paths_ready(h, "gpmpc_paths_eval_grid"));
    if (B <= 0 || !Z || !f) return fail(GPMPC_EINVAL, "bad B or NULL Z / f");
    HIPCHK(hipSetDevice(h->device));
    CHK(ensure_scratch(h, B));
    const int S = h->pS, Sld = h->pSld, F = h->pF, Fp = h->pFp, d = h->d, Ny = h->Ny, N = h->N, Np = h->Np;
    const int step = chunk_step(h), Bpmax = round_up(std::min(B, step), 32);
    DevArena mem;
    double* G = mem.take<double>((size_t)Ny * Sld * Bpmax);
    double* PhiZ = mem.take<double>((size_t)Ny * Bpmax * Fp);
    double* dF = mem.take<double>((size_t)S * B * Ny);
    if (mem.status != hipSuccess) {
        (void)hipGetLastError();
        return fail(GPMPC_ENOMEM, "gpmpc_paths_eval_grid: no device memory for %d x %d x %d results", S, B, Ny);
    }
    const Ctx cx = h->cx();
    hipStream_t st = h->stream;
    const bool madd = h->mean_kind && h->mean_add;
    for (int b0 = 0; b0 < B; b0 += step) {
        const int nb = std::min(step, B - b0), Bp = round_up(nb, 32);
        HIPCHK(hipMemcpyAsync(h->Z, Z + (size_t)b0 * d, (size_t)nb * d * sizeof(double), hipMemcpyHostToDevice, st));
        ProfScope t(&h->prof, st, GPMPC_PH_MC);
        launch_crosscov(st, d, h->XT, h->ws.hyper, nullptr, h->Z, h->KsT, h->meanT, nullptr, N, Np, nb, Bp, Ny);
        hipLaunchKernelGGL(paths_phi_kernel, dim3((unsigned)(((size_t)Ny * Bp * (Fp / 2) + 255) / 256)), dim3(256), 0, st, h->Z, (long)d,
                           1L, h->pOmega, h->ws.hyper, PhiZ, Ny, nb, Bp, F, Fp, d);
        GemmP g = gemm_base(cx);                        // G[s][b] = sum_i V[i][s] Ks[b][i]
        g.A = h->pV; g.lda = Sld; g.sA = (long)Np * Sld; g.a_mc = 1;
        g.B = h->KsT; g.ldb = Np; g.sB = (long)Bp * Np; g.b_nc = 0;
        g.C = G; g.ldc = Bp; g.sC = (long)Sld * Bp;
        g.M = Sld; g.N = Bp; g.K = Np;
        launch_gemm(g, Ny, st);
        GemmP q = gemm_base(cx);                        // G[s][b] += sum_j WT[j][s] Phi(Z)[b][j]
        q.A = h->pWT; q.lda = Sld; q.sA = (long)Fp * Sld; q.a_mc = 1;
        q.B = PhiZ; q.ldb = Fp; q.sB = (long)Bp * Fp; q.b_nc = 0;
        q.C = G; q.ldc = Bp; q.sC = (long)Sld * Bp;
        q.M = Sld; q.N = Bp; q.K = Fp; q.beta = 1.0;
        launch_gemm(q, Ny, st);
        hipLaunchKernelGGL(paths_grid_out_kernel, dim3((unsigned)(((size_t)S * nb * Ny + 255) / 256)), dim3(256), 0, st, G,
                           (long)Sld * Bp, (long)Bp, h->Z, h->mpar, madd ? h->mean_kind : 0, dF, S, nb, b0, B, Ny, d);
    }
    hipError_t e = hipMemcpyAsync(f, dF, (size_t)S * B * Ny * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GPMPC_EHIP, "%s", hipGetErrorString(e));
    return GPMPC_OK;
}

extern "C" int gpmpc_rollout_paths(gpmpc_gp* h, int T, unsigned long long seed, int noise, const double* z0, const double* Sigma0,
                                   const double* U, const double* sa, const double* sb, const double* Kz, const double* k0,
                                   const double* eps0, const double* eps, double* mean, double* cov, double* particles) {
    CHK(paths_ready(h, "gpmpc_rollout_paths"));
    const int S = h->pS, d = h->d, Ny = h->Ny, Nu = d - Ny;
    const bool fb = Kz != nullptr;
    if (T <= 0 || !z0 || !Sigma0 || !mean || !cov || (!fb && Nu > 0 && !U)) return fail(GPMPC_EINVAL, "bad T or NULL argument");
    if (Nu < 0) return fail(GPMPC_EINVAL, "roll-out needs d >= Ny (inputs are [state, control])");
    if (fb && (Nu == 0 || !k0)) return fail(GPMPC_EINVAL, "feedback roll-out needs controls and Kz, k0");
    double L0[DMAX * DMAX];
    if (!chol_semidefinite(Sigma0, d, L0)) return fail(GPMPC_EINVAL, "Sigma0 is not positive semidefinite");
    HIPCHK(hipSetDevice(h->device));
    CHK(paths_part_reserve(h));
    if (!noise) eps = nullptr;                                      // (nothing is drawn after step 0)
    // the device block of gpmpc_rollout_mc, without the prediction's mean / variance scratch: one copy up, one copy down
    const int nu1 = std::max(Nu, 1), nblk = (S + MC_BLOCK - 1) / MC_BLOCK, P = Ny * (Ny + 1) / 2;
    const size_t nz = d, nL = (size_t)d * d, nK = (size_t)nu1 * Ny, nU = (size_t)T * nu1, nSy = (size_t)S * Ny;
    const size_t nE0 = eps0 ? (size_t)S * d : 0, nE = eps ? (size_t)T * nSy : 0;
    auto even = [](size_t n) { return (n + 1) & ~(size_t)1; };
    const size_t nIn = even(nz + nL + 2 * Ny + nK + nu1 + nU + nE0 + nE), nZp = even((size_t)S * d);
    const size_t nScr = nZp + (particles ? 0 : nSy) + (size_t)nblk * P;
    const size_t nM = (size_t)T * Ny, nC = (size_t)T * Ny * Ny, nP = particles ? (size_t)T * nSy : 0, nOut = nM + nC + nP;
    CHK(paths_io_reserve(h, nIn + nScr + nOut, nIn + nOut));
    double* buf = h->pio_dev;
    double *dz = buf, *dL = dz + nz, *dsa = dL + nL, *dsb = dsa + Ny, *dKz = dsb + Ny, *dk0 = dKz + nK, *dU = dk0 + nu1,
           *dE0 = dU + nU, *dE = dE0 + nE0;
    double *dZp = buf + nIn, *dY = dZp + nZp, *dPart = dY + (particles ? 0 : nSy);
    double *dM = buf + nIn + nScr, *dC = dM + nM, *dP = dC + nC;
    {
        double* pz = h->pio_pin;
        auto put = [&](double* dev_dst, const double* src, size_t n) { std::memcpy(pz + (dev_dst - buf), src, n * sizeof(double)); };
        std::memset(pz, 0, (size_t)(dE0 - buf) * sizeof(double));
        put(dz, z0, nz);
        put(dL, L0, nL);
        for (int a = 0; a < Ny; ++a) pz[(dsa - buf) + a] = sa ? sa[a] : 1.0;
        if (sb) put(dsb, sb, Ny);
        if (fb) {
            put(dKz, Kz, nK);
            put(dk0, k0, Nu);
        } else if (Nu > 0) {
            put(dU, U, nU);
        }
        if (eps0) put(dE0, eps0, nE0);
        if (eps) put(dE, eps, nE);
    }
    HIPCHK(hipMemcpyAsync(buf, h->pio_pin, nIn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const dim3 pgrid((unsigned)nblk), pblock(MC_BLOCK);
    const bool madd = h->mean_kind && h->mean_add;
    const int nparts = paths_part_blocks(h->N, h->pF);
    {
        ProfScope pt(&h->prof, h->stream, GPMPC_PH_MC);
        hipLaunchKernelGGL(mc_init_kernel, pgrid, pblock, 0, h->stream, dz, dL, eps0 ? dE0 : (const double*)nullptr, seed, dZp, S, d);
        for (int t = 0; t < T; ++t) {
            double* Yt = particles ? dP + (size_t)t * nSy : dY;
            const bool last = t + 1 == T;
            paths_eval_launch(h, dZp);
            hipLaunchKernelGGL(paths_finish_kernel, pgrid, pblock, 0, h->stream, h->pPart, nparts, dZp, h->mpar, madd ? h->mean_kind : 0,
                               h->ws.hyper, noise ? 1 : 0, eps ? dE + (size_t)t * nSy : (const double*)nullptr, seed, (unsigned)(1 + t),
                               Yt, last ? (double*)nullptr : dZp, dsa, dsb, last ? (const double*)nullptr : dU + (size_t)(t + 1) * nu1,
                               fb ? dKz : (const double*)nullptr, fb ? dk0 : (const double*)nullptr, S, h->pSld, Ny, d);
            double* oM = dM + (size_t)t * Ny;
            hipLaunchKernelGGL(mc_moments_partial_kernel, pgrid, pblock, 0, h->stream, Yt, (const double*)nullptr, dPart, S, Ny);
            hipLaunchKernelGGL(mc_moments_final_kernel, dim3(Ny), pblock, 0, h->stream, dPart, nblk, Ny, 1.0 / S, oM, 0, Ny);
            hipLaunchKernelGGL(mc_moments_partial_kernel, pgrid, pblock, 0, h->stream, Yt, oM, dPart, S, Ny);
            hipLaunchKernelGGL(mc_moments_final_kernel, dim3(P), pblock, 0, h->stream, dPart, nblk, P, S > 1 ? 1.0 / (S - 1) : 0.0,
                               dC + (size_t)t * Ny * Ny, 1, Ny);
        }
    }
    double* pout = h->pio_pin + nIn;
    hipError_t e = hipMemcpyAsync(pout, dM, nOut * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GPMPC_EHIP, "%s", hipGetErrorString(e));
    std::memcpy(mean, pout, nM * sizeof(double));
    std::memcpy(cov, pout + nM, nC * sizeof(double));
    if (particles) std::memcpy(particles, pout + nM + nC, nP * sizeof(double));
    return GPMPC_OK;
}
