// api_mc.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: Monte Carlo roll-outs: S particles through the GP for T steps on the device (mc_kernels.hpp), gpmpc_randn.

// Lower-triangular L with L L^T = A for a symmetric positive SEMIdefinite A[n x n] (its lower triangle is read): a pivot
// within n eps max(diag) of zero gives a zero column (a deterministic direction, e.g. exactly known controls), provided the
// rest of that column vanishes as well (|a_ij|^2 <= a_ii a_jj for a semidefinite matrix).  false: A is not semidefinite.
static bool chol_semidefinite(const double* A, int n, double* L) {
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!(A[i * n + i] == A[i * n + i])) return false;
        dmax = std::max(dmax, A[i * n + i]);
    }
    const double tol = n * 2.220446049250313e-16 * dmax;
    std::fill(L, L + (size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double p = A[j * n + j];
        for (int k = 0; k < j; ++k) p -= L[j * n + k] * L[j * n + k];
        if (!(p >= -tol)) return false;                        // clearly negative (or NaN)
        const bool zero = p <= tol;
        const double ljj = zero ? 0.0 : std::sqrt(p);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double r = A[i * n + j];
            for (int k = 0; k < j; ++k) r -= L[i * n + k] * L[j * n + k];
            if (zero) {
                if (!(std::fabs(r) <= 2.0 * std::sqrt(tol * dmax))) return false;
            } else {
                L[i * n + j] = r / ljj;
            }
        }
    }
    return true;
}

extern "C" int gpmpc_rollout_mc(gpmpc_gp* h, int S, int T, unsigned long long seed, int noise, const double* z0,
                                const double* Sigma0, const double* U, const double* sa, const double* sb, const double* Kz,
                                const double* k0, const double* eps0, const double* eps, double* mean, double* cov,
                                double* particles) {
    if (!h) return fail(GPMPC_EINVAL, "NULL handle");
    if (!h->fitted) return fail(GPMPC_ENOTFIT, "model has no factors (call gpmpc_fit or gpmpc_set_factors)");
    const int d = h->d, Ny = h->Ny, Nu = d - Ny;
    const bool fb = Kz != nullptr;
    if (S < 1 || S > (1 << 20)) return fail(GPMPC_EINVAL, "bad S = %d (1 .. 2^20 particles)", S);
    if (T <= 0 || !z0 || !Sigma0 || !mean || !cov || (!fb && Nu > 0 && !U)) return fail(GPMPC_EINVAL, "bad T or NULL argument");
    if (Nu < 0) return fail(GPMPC_EINVAL, "roll-out needs d >= Ny (inputs are [state, control])");
    if (fb && (Nu == 0 || !k0)) return fail(GPMPC_EINVAL, "feedback roll-out needs controls and Kz, k0");
    double L0[DMAX * DMAX];
    if (!chol_semidefinite(Sigma0, d, L0)) return fail(GPMPC_EINVAL, "Sigma0 is not positive semidefinite");
    HIPCHK(hipSetDevice(h->device));
    CHK(ensure_scratch(h, S));
    // device block (grow-only, with a pinned mirror of its two ends): the inputs [z0 | L0 | sa | sb | Kz | k0 | U | eps0 | eps],
    // scratch [particle inputs | mean | var | y of the step | partial sums], the results [mean (T) | cov (T) | particles]:
    // one copy up, one copy down
    const int nu1 = std::max(Nu, 1), nblk = (S + MC_BLOCK - 1) / MC_BLOCK, P = Ny * (Ny + 1) / 2;
    const size_t nz = d, nL = (size_t)d * d, nK = (size_t)nu1 * Ny, nU = (size_t)T * nu1, nSy = (size_t)S * Ny;
    const size_t nE0 = eps0 ? (size_t)S * d : 0, nE = eps ? (size_t)T * nSy : 0;
    auto even = [](size_t n) { return (n + 1) & ~(size_t)1; };      // what predict_chunk reads and writes stays 16-byte aligned
    const size_t nIn = even(nz + nL + 2 * Ny + nK + nu1 + nU + nE0 + nE), nZp = even((size_t)S * d), nSyE = even(nSy);
    const size_t nScr = nZp + 2 * nSyE + (particles ? 0 : nSy) + (size_t)nblk * P;
    const size_t nM = (size_t)T * Ny, nC = (size_t)T * Ny * Ny, nP = particles ? (size_t)T * nSy : 0, nOut = nM + nC + nP;
    if (nIn + nScr + nOut > h->mc_cap || nIn + nOut > h->mc_pin_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        hipFree(h->mc_dev);
        if (h->mc_pin) hipHostFree(h->mc_pin);
        h->mc_dev = h->mc_pin = nullptr;
        const size_t cap = std::max(h->mc_cap, nIn + nScr + nOut), pin_cap = std::max(h->mc_pin_cap, nIn + nOut);
        h->mc_cap = h->mc_pin_cap = 0;
        HIPCHK(hipMalloc(&h->mc_dev, cap * sizeof(double)));
        HIPCHK(hipHostMalloc((void**)&h->mc_pin, pin_cap * sizeof(double), hipHostMallocDefault));
        h->mc_cap = cap;
        h->mc_pin_cap = pin_cap;
    }
    double* buf = h->mc_dev;
    double *dz = buf, *dL = dz + nz, *dsa = dL + nL, *dsb = dsa + Ny, *dKz = dsb + Ny, *dk0 = dKz + nK, *dU = dk0 + nu1,
           *dE0 = dU + nU, *dE = dE0 + nE0;
    double *dZp = buf + nIn, *dPm = dZp + nZp, *dPv = dPm + nSyE, *dY = dPv + nSyE, *dPart = dY + (particles ? 0 : nSy);
    double *dM = buf + nIn + nScr, *dC = dM + nM, *dP = dC + nC;
    {
        double* pz = h->mc_pin;
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
    HIPCHK(hipMemcpyAsync(buf, h->mc_pin, nIn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const dim3 pgrid((unsigned)nblk), pblock(MC_BLOCK);
    {
        ProfScope t(&h->prof, h->stream, GPMPC_PH_MC);
        hipLaunchKernelGGL(mc_init_kernel, pgrid, pblock, 0, h->stream, dz, dL, eps0 ? dE0 : (const double*)nullptr, seed, dZp, S, d);
    }
    const int step = chunk_step(h);
    int rc = GPMPC_OK;
    for (int t = 0; t < T && rc == GPMPC_OK; ++t) {
        for (int b0 = 0; b0 < S && rc == GPMPC_OK; b0 += step) {
            const int nb = std::min(step, S - b0);
            rc = predict_chunk(h, nb, dZp + (size_t)b0 * d, dPm + (size_t)b0 * Ny, dPv + (size_t)b0 * Ny, nullptr);
        }
        if (rc != GPMPC_OK) break;
        ProfScope pt(&h->prof, h->stream, GPMPC_PH_MC);
        double* Yt = particles ? dP + (size_t)t * nSy : dY;
        const bool last = t + 1 == T;
        hipLaunchKernelGGL(mc_step_kernel, pgrid, pblock, 0, h->stream, dPm, dPv, h->ws.hyper, noise ? 1 : 0,
                           eps ? dE + (size_t)t * nSy : (const double*)nullptr, seed, (unsigned)(1 + t), Yt,
                           last ? (double*)nullptr : dZp, dsa, dsb, last ? (const double*)nullptr : dU + (size_t)(t + 1) * nu1,
                           fb ? dKz : (const double*)nullptr, fb ? dk0 : (const double*)nullptr, S, Ny, d);
        double* oM = dM + (size_t)t * Ny;
        hipLaunchKernelGGL(mc_moments_partial_kernel, pgrid, pblock, 0, h->stream, Yt, (const double*)nullptr, dPart, S, Ny);
        hipLaunchKernelGGL(mc_moments_final_kernel, dim3(Ny), pblock, 0, h->stream, dPart, nblk, Ny, 1.0 / S, oM, 0, Ny);
        hipLaunchKernelGGL(mc_moments_partial_kernel, pgrid, pblock, 0, h->stream, Yt, oM, dPart, S, Ny);
        hipLaunchKernelGGL(mc_moments_final_kernel, dim3(P), pblock, 0, h->stream, dPart, nblk, P, S > 1 ? 1.0 / (S - 1) : 0.0,
                           dC + (size_t)t * Ny * Ny, 1, Ny);
    }
    if (rc != GPMPC_OK) {
        hipStreamSynchronize(h->stream);
        return rc;
    }
    double* pout = h->mc_pin + nIn;
    hipError_t e = hipMemcpyAsync(pout, dM, nOut * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GPMPC_EHIP, "%s", hipGetErrorString(e));
    std::memcpy(mean, pout, nM * sizeof(double));
    std::memcpy(cov, pout + nM, nC * sizeof(double));
    if (particles) std::memcpy(particles, pout + nM + nC, nP * sizeof(double));
    return GPMPC_OK;
}

extern "C" int gpmpc_randn(int device, unsigned long long seed, unsigned stream, int rows, int cols, double* out) {
    if (rows < 1 || cols < 1 || !out || (long)rows * cols > (1L << 31)) return fail(GPMPC_EINVAL, "bad rows / cols or NULL out");
    CHK(ensure_device(device));
    DevArena mem;
    const size_t n = (size_t)rows * cols;
    double* dv = mem.take<double>(n);
    HIPCHK(mem.status);
    const long threads = (long)rows * ((cols + 1) / 2);
    hipLaunchKernelGGL(mc_randn_kernel, dim3((unsigned)((threads + MC_BLOCK - 1) / MC_BLOCK)), dim3(MC_BLOCK), 0, 0, seed, stream, rows,
                       cols, dv);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dv, n * sizeof(double), hipMemcpyDeviceToHost));
    return GPMPC_OK;
}
