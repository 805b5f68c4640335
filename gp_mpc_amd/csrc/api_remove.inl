// api_remove.inl -- part of gpmpc_api.hip (one translation unit; included in order, not compiled alone).
// Concern: gpmpc_remove -- take training points out of the model: Householder downdate of L and L^-1 on the device
// (remove_kernels.hpp), or a refit on the remaining rows where the downdate cannot pay.
// ------------------------------------------------------------------------------------------------
static int g_remove_mode = -1;      // gpmpc_set_tuning("remove_mode", 0 / 1 / 2): automatic / always downdate / always refit; -1: default (automatic)

// The automatic rule: a cost model whose constants are read off profiles/remove_vs_refit.txt (MI355X, whole calls, microseconds).
//   downdate, per pass of m <= REMOVE_W points into Np padded rows:  fixed host + allocation cost, the compaction of L and L^-1
//     (bytes ~ Ny Np^2), and per 64-column panel from the first removed index on one (panel, apply) launch pair -- the panel
//     kernel's 64 sequential reflectors dominate it (55 / 100 / 205 us at item widths 4 / 16 / 64), the apply kernel adds a
//     term in the number of items;
//   refit: a fixed part and the N^3 flops of the factorisation and the inverse.
// More than a quarter of the remaining size always refits, as gpmpc_append does for its large n: there the downdate's
// O(N^2 n) is no fewer flops than the fit's O(N^3).
static bool remove_prefers_downdate(int N1, int Ny, const std::vector<int>& sorted_idx) {
    const int n = (int)sorted_idx.size();
    if (4L * n > N1) return false;
    double downdate_us = 0.0;
    for (int hi = n, Ncur = N1 + n; hi > 0; hi -= REMOVE_W) {     // the passes of gpmpc_remove, highest indices first
        const int lo = std::max(hi - REMOVE_W, 0), m = hi - lo, Nn = Ncur - m;
        const double np = round_up(Nn, 64), panels = std::max(0, (Nn + 63) / 64 - sorted_idx[lo] / 64);
        const double panel_us = m <= 4 ? 55.0 : m <= 16 ? 100.0 : 205.0;
        downdate_us += 750.0 + 150.0 * Ny + 1.0e-5 * Ny * np * np + panels * (panel_us + 3.3e-3 * np * (1.0 + 0.42 * (Ny - 1)));
        Ncur = Nn;
    }
    const double np1 = round_up(N1, 64);
    const double refit_us = 1150.0 + 150.0 * Ny + 1.9e-8 * Ny * np1 * np1 * np1;
    return downdate_us < refit_us;
}

namespace {
struct RemoveScratch {              // device scratch of one call; released on every way out
    DevArena mem;                   // owns Et .. rem below
    double *Et = nullptr, *G = nullptr, *V = nullptr, *tau = nullptr;
    int *src = nullptr, *rem = nullptr;
    double *pL[2] = {nullptr, nullptr}, *pT[2] = {nullptr, nullptr};   // intermediate factors: device block list (block_alloc)
    ~RemoveScratch() {
        for (int s = 0; s < 2; ++s) { block_free(pL[s]); block_free(pT[s]); }
    }
};
// what the call builds beside the old model; handed to the handle at the end, released on any earlier way out
struct RemoveNew {
    double *XT = nullptr, *Y = nullptr;
    Workspace ws;
    bool keep = false;
    ~RemoveNew() {
        if (keep) return;
        hipFree(XT); hipFree(Y);
        ws_free(ws);
    }
};
}  // namespace

template <int NX>
static void remove_launch_panels(hipStream_t st, int Ny, double* L1, double* T1, double* Et, double* G, int Np1, int N1, int p0,
                                 double* V, double* tau) {
    for (int p = p0; 64 * p < N1; ++p) {
        hipLaunchKernelGGL((remove_panel_kernel<NX>), dim3(Ny), dim3(256), 0, st, L1, Et, Np1, p, V, tau);
        const int items = std::min(64 * (p + 1), N1) + std::max(N1 - 64 * (p + 1), 0);
        hipLaunchKernelGGL((remove_apply_kernel<NX>), dim3((items + 63) / 64, Ny), dim3(64), 0, st, L1, T1, Et, G, Np1, N1, p, V, tau);
    }
}

// One pass: the factors (L0, T0) of N0 points, leading dimension Np0, without the points rem[0 .. n) (ascending, n <= REMOVE_W)
// into (L1, T1), leading dimension Np1 = round_up(N0 - n, 64).  Enqueues only; s.src / s.rem are filled with blocking copies.
static int remove_pass(hipStream_t st, int Ny, const double* L0, const double* T0, int Np0, int N0, double* L1, double* T1,
                       int Np1, const int* rem, int n, bool zero_upper, RemoveScratch& s) {
    const int N1 = N0 - n;
    std::vector<int> src(Np1, -1);
    for (int i = 0, o = 0, k = 0; o < N0; ++o) {
        if (k < n && rem[k] == o) { ++k; continue; }
        src[i++] = o;
    }
    HIPCHK(hipMemcpy(s.src, src.data(), (size_t)Np1 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.rem, rem, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    const int NX = n <= 4 ? 4 : n <= 16 ? 16 : 64;
    double *Et = s.Et, *G = s.G, *V = s.V, *tau = s.tau;
    const int *dsrc = s.src, *drem = s.rem;
    hipLaunchKernelGGL(remove_gather_kernel, dim3(Np1 + 2 * NX, (Np1 + 255) / 256, Ny), dim3(256), 0, st, L0, T0, Np0, L1, T1, Np1,
                       Et, G, dsrc, drem, n, NX, zero_upper ? 1 : 0);
    const int p0 = rem[0] / 64;                             // columns below 64 p0 do not change
    if (NX == 4) remove_launch_panels<4>(st, Ny, L1, T1, Et, G, Np1, N1, p0, V, tau);
    else if (NX == 16) remove_launch_panels<16>(st, Ny, L1, T1, Et, G, Np1, N1, p0, V, tau);
    else remove_launch_panels<64>(st, Ny, L1, T1, Et, G, Np1, N1, p0, V, tau);
    HIPCHK(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_remove(gpmpc_gp* h, int n, const int* idx) {
    if (!h || !idx) return fail(GPMPC_EINVAL, "NULL handle or idx");
    CHK(refuse_sparse(h, "gpmpc_remove"));
    if (n <= 0 || n >= h->N) return fail(GPMPC_EINVAL, "remove: need 1 <= n < N (n = %d, N = %d)", n, h->N);
    std::vector<int> rem(idx, idx + n);
    std::sort(rem.begin(), rem.end());
    if (rem.front() < 0 || rem.back() >= h->N) return fail(GPMPC_EINVAL, "remove: index out of range [0, %d)", h->N);
    for (int k = 1; k < n; ++k)
        if (rem[k] == rem[k - 1]) return fail(GPMPC_EINVAL, "remove: index %d is listed twice", rem[k]);
    if (!h->fitted) return fail(GPMPC_ENOTFIT, "model has no factors (call gpmpc_fit or gpmpc_set_factors)");
    HIPCHK(hipSetDevice(h->device));
    alpha_ready(h);
    h->tail.armed = false;
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N0 = h->N, N1 = N0 - n, d = h->d, Ny = h->Ny, Np0 = h->Np, Np1 = round_up(N1, 64);
    const bool downdate = g_remove_mode == 1 || (g_remove_mode != 2 && remove_prefers_downdate(N1, Ny, rem));
    // new data buffers: the kept points in their order
    RemoveNew nw;
    {
        std::vector<double> xt0((size_t)d * Np0), yt0((size_t)Ny * Np0), xt((size_t)d * Np1, 0.0), yt((size_t)Ny * Np1, 0.0);
        HIPCHK(hipMemcpy(xt0.data(), h->XT, xt0.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(yt0.data(), h->Y, yt0.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0, o = 0, k = 0; o < N0; ++o) {
            if (k < n && rem[k] == o) { ++k; continue; }
            for (int c = 0; c < d; ++c) xt[(size_t)c * Np1 + i] = xt0[(size_t)c * Np0 + o];
            for (int a = 0; a < Ny; ++a) yt[(size_t)a * Np1 + i] = yt0[(size_t)a * Np0 + o];
            ++i;
        }
        HIPCHK(hipMalloc(&nw.XT, xt.size() * sizeof(double)));
        HIPCHK(hipMalloc(&nw.Y, yt.size() * sizeof(double)));
        HIPCHK(hipMemcpy(nw.XT, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(nw.Y, yt.data(), yt.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    CHK(ws_alloc(nw.ws, Ny, Np1, d));
    HIPCHK(hipMemcpy(nw.ws.hyper, h->ws.hyper, (size_t)Ny * (d + 2) * sizeof(double), hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(nw.ws.jitter, h->ws.jitter, (size_t)Ny * sizeof(double), hipMemcpyDeviceToDevice));
    h->nll_last_a = -1;                                     // (the training workspace's factors belong to the old data)
    if (!downdate) {                                        // plain refit, with gpmpc_append's rollback discipline
        double *XT0 = h->XT, *Y0 = h->Y;
        Workspace ws0 = h->ws;
        const bool invK0 = h->have_invK;
        const std::vector<double> hy = h->hyper;
        free_predict_scratch(h);
        h->XT = nw.XT; h->Y = nw.Y; h->ws = nw.ws;
        h->N = N1; h->Np = Np1;
        nw.keep = true;
        const int rc = gpmpc_fit(h, hy.data(), 0, nullptr);
        if (rc == GPMPC_OK) {
            hipFree(XT0); hipFree(Y0);
            ws_free(ws0);
            ++h->n_remove_refit;
            return GPMPC_OK;
        }
        const std::string keep = g_err;
        hipStreamSynchronize(h->stream);
        ws_free(h->ws);
        hipFree(h->XT); hipFree(h->Y);
        h->XT = XT0; h->Y = Y0; h->ws = ws0;
        h->N = N0; h->Np = Np0;
        h->hyper = hy;
        h->fitted = true;
        h->have_invK = invK0;
        h->have_beta = false;
        ++h->factor_gen;
        refresh_residual(h);
        g_err = keep;
        return rc;
    }
    // passes of at most REMOVE_W points, the highest indices first (the lower ones keep their numbers); all but the last
    // pass write to one of two scratch pairs, the last one to the new workspace
    const int passes = (n + REMOVE_W - 1) / REMOVE_W;
    RemoveScratch s;
    {
        const int NpA = round_up(N0 - std::min(n, REMOVE_W), 64);   // the largest result
        const size_t xb = (size_t)Ny * REMOVE_W * NpA;
        s.Et = s.mem.take<double>(xb);
        s.G = s.mem.take<double>(xb);
        s.V = s.mem.take<double>((size_t)Ny * 64 * REMOVE_W);
        s.tau = s.mem.take<double>((size_t)Ny * 64);
        s.src = s.mem.take<int>((size_t)NpA);
        s.rem = s.mem.take<int>((size_t)REMOVE_W);
        HIPCHK(s.mem.status);
        for (int q = 0; q < std::min(passes - 1, 2); ++q) {
            const int NpQ = round_up(N0 - std::min(n, (q + 1) * REMOVE_W), 64);
            HIPCHK(block_alloc(&s.pL[q], (size_t)Ny * NpQ * NpQ * sizeof(double)));
            HIPCHK(block_alloc(&s.pT[q], (size_t)Ny * NpQ * NpQ * sizeof(double)));
        }
    }
    const double *Lc = h->ws.L, *Tc = h->ws.Inv;
    int Nc = N0, Npc = Np0;
    for (int q = 0, hi = n; q < passes; ++q) {
        const int lo = std::max(hi - REMOVE_W, 0), Nn = Nc - (hi - lo), Npn = round_up(Nn, 64);
        const bool last = q == passes - 1;
        double* Ln = last ? nw.ws.L : s.pL[q & 1];
        double* Tn = last ? nw.ws.Inv : s.pT[q & 1];
        if (q > 0) HIPCHK(hipStreamSynchronize(h->stream));     // (the pass before still reads the index maps)
        CHK(remove_pass(h->stream, Ny, Lc, Tc, Npc, Nc, Ln, Tn, Npn, rem.data() + lo, hi - lo, !last, s));
        Lc = Ln; Tc = Tn; Nc = Nn; Npc = Npn;
        hi = lo;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    // the handle takes the new data set
    hipFree(h->XT); hipFree(h->Y);
    ws_free(h->ws);
    free_predict_scratch(h);
    h->XT = nw.XT; h->Y = nw.Y; h->ws = nw.ws;
    nw.keep = true;
    h->N = N1; h->Np = Np1;
    ++h->factor_gen;                                        // (drawn paths belong to the old data: api_paths.inl)
    h->have_invK = false;
    ++h->n_remove_down;
    CHK(refresh_residual(h));
    solve_alpha(h->cx(), h->ws, h->y_model(), h->Np);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return GPMPC_OK;
}
