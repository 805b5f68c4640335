// select_kernels.hpp -- greedy max-variance selection of new training points (gpmpc_append_select, api_select.inl).
//
// From n candidates C the k most informative ones, one at a time: the pick of step t is the candidate whose noise-free
// predictive variance, summed over the outputs, is largest given the training data AND the t points picked before.  What
// the reference's GP.update_data set out to do (gp_class.py:384-471; its arg-min / norm slips are documented there).
//
// Per output a the candidates' posterior covariance S_a = k_a(C, C) - V^T V, V = L_a^-1 k_a(X, C), is formed ONCE (the GEMMs
// of gpmpc_covar).  Adding the noisy observation at candidate p to the model changes every candidate's variance by
//     var(j) -= S[j][p]^2 / (S[p][p] + sn^2 + jitter)
// and S itself by the corresponding rank-1 term: a Cholesky step on S whose pivot carries the noise (the point enters K with
// k(x, x) + sn^2, gp_class.py:440) while the scores stay noise-free.  So k steps of a partial Cholesky with the pivot chosen
// jointly over the outputs give the picks; the N x N factors are never touched again.
//   state per output: dg_a[j] running variance, G_a[:, t] = pivot columns (stored column by column: GT[a][t][Bp])
//   step t:  p = argmax_j sum_a dg_a[j];   c = S_a[:, p] - G_a[:, :t] G_a[p, :t];   g = c / sqrt(dg_a[p] + sn_a^2 + jitter_a);
//            G_a[:, t] = g;   dg_a[j] = max(dg_a[j] - g_j^2, 0)
// One launch per step, Bp / 64 workgroups; stream order is the only synchronisation between steps, no workgroup waits for
// another one.  Every workgroup re-derives the arg-max from the score vector the previous launch left in memory -- a pure
// function of that vector (largest value, lowest index among equals; the comparison is a total order, so the reduction tree
// cannot change the outcome).  dg / score are double-buffered by the parity of t: a launch reads what its predecessor wrote
// and writes the other copy, so no workgroup reads an entry another one of the same launch writes.
#pragma once
#include <hip/hip_runtime.h>

namespace gpmpc {

// S[a][i][j] = sf_a^2 exp(-1/2 sum_d (c_i,d - c_j,d)^2 / ell_a,d^2) + S[a][i][j] for i, j < n (S holds -V^T V on entry), 0 in
// the padding.  The direct-difference form: the diagonal is sf^2 exactly, as in gpmpc_covar.  grid (Bp / 256 rounded up, Bp, Ny).
__global__ void __launch_bounds__(256) select_schur_kernel(const double* __restrict__ Z, const double* __restrict__ hyper,
                                                           double* __restrict__ S, int n, int Bp, int d) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x, i = blockIdx.y, a = blockIdx.z;
    if (j >= Bp) return;
    const double* hy = hyper + (long)a * (d + 2);
    double* s = S + ((long)a * Bp + i) * Bp + j;
    if (i >= n || j >= n) { *s = 0.0; return; }
    double dist = 0.0;
    for (int dd = 0; dd < d; ++dd) {
        const double df = (Z[(long)i * d + dd] - Z[(long)j * d + dd]) / hy[dd];
        dist = fma(df, df, dist);
    }
    *s = hy[d] * hy[d] * exp(-0.5 * dist) + *s;
}

// dg[0][a][j] = max(S_a[j][j], 0), score[0][j] = sum_a dg[0][a][j] (outputs added in order); padding: 0 and -1.
// A score < 0 marks an entry that cannot be picked (padding, and later the picked ones).  grid (Bp / 256 rounded up).
__global__ void __launch_bounds__(256) select_init_kernel(const double* __restrict__ S, double* __restrict__ dg,
                                                          double* __restrict__ score, int n, int Bp, int Ny) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= Bp) return;
    double tot = 0.0;
    for (int a = 0; a < Ny; ++a) {
        const double v = j < n ? fmax(S[((long)a * Bp + j) * Bp + j], 0.0) : 0.0;
        dg[(long)a * Bp + j] = v;
        tot += v;
    }
    score[j] = j < n ? tot : -1.0;
}

__device__ __forceinline__ bool select_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// Step t.  grid (Bp / 64), 256 threads: lane l of every wave owns candidate row 64 blockIdx.x + l, the four waves split the
// t earlier pivot columns (column s goes to wave s mod 4) and their partial dot products are added in a fixed order.
// flags: [0] the number of picks made so far (workgroup 0), [1 + t] "selection stopped before step t" -- launch t reads
// [1 + t] and writes [2 + t], so the early stop turns every later launch into a no-op without a host round trip.
__global__ void __launch_bounds__(256) select_step_kernel(const double* __restrict__ S, double* __restrict__ GT,
                                                          double* __restrict__ dg, double* __restrict__ score,
                                                          const double* __restrict__ hyper, const double* __restrict__ jitter,
                                                          int* __restrict__ selected, double* __restrict__ gain,
                                                          int* __restrict__ flags, int n, int Bp, int k, int Ny, int d, int t,
                                                          double min_gain) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double bval[256];
    __shared__ int bidx[256];
    __shared__ double red[4][64];
    if (flags[1 + t]) {
        if (blockIdx.x == 0 && tid == 0) flags[2 + t] = 1;
        return;
    }
    const double* __restrict__ sc = score + (long)(t & 1) * Bp;
    double* __restrict__ sc_next = score + (long)((t + 1) & 1) * Bp;
    const double* __restrict__ dg_cur = dg + (long)(t & 1) * Ny * Bp;
    double* __restrict__ dg_next = dg + (long)((t + 1) & 1) * Ny * Bp;
    // arg-max of the scores: largest value, lowest index among equals; entries < 0 (picked, padding) and NaN never win
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int j = tid; j < n; j += 256) {
        const double v = sc[j];
        if (v >= 0.0 && select_better(v, j, bv, bi)) { bv = v; bi = j; }
    }
    bval[tid] = bv;
    bidx[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && select_better(bval[tid + w], bidx[tid + w], bval[tid], bidx[tid])) {
            bval[tid] = bval[tid + w];
            bidx[tid] = bidx[tid + w];
        }
        __syncthreads();
    }
    const double best = bval[0];
    const int p = bidx[0];
    if (p >= n || (min_gain > 0.0 && best < min_gain)) {      // nothing left to pick, or not worth a pick: stop here
        if (blockIdx.x == 0 && tid == 0) flags[2 + t] = 1;
        return;
    }
    if (blockIdx.x == 0 && tid == 0) {
        selected[t] = p;
        gain[t] = best;
        flags[0] = t + 1;
    }
    const int j = (int)blockIdx.x * 64 + lane;
    double tot = 0.0;
    for (int a = 0; a < Ny; ++a) {
        const double* __restrict__ Ga = GT + (long)a * k * Bp;
        double part = 0.0;
        for (int s = wave; s < t; s += 4) part = fma(Ga[(long)s * Bp + j], Ga[(long)s * Bp + p], part);
        red[wave][lane] = part;
        __syncthreads();
        if (wave == 0) {
            const double dot = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
            const double* hy = hyper + (long)a * (d + 2);
            const double piv = (dg_cur[(long)a * Bp + p] + hy[d + 1] * hy[d + 1]) + jitter[a];
            const double c = S[((long)a * Bp + p) * Bp + j] - dot;           // (row p of the symmetric S: coalesced)
            const double g = (j < n && piv > 0.0) ? c / sqrt(piv) : 0.0;
            GT[((long)a * k + t) * Bp + j] = g;
            const double v = fmax(dg_cur[(long)a * Bp + j] - g * g, 0.0);
            dg_next[(long)a * Bp + j] = v;
            tot += v;
        }
        __syncthreads();
    }
    if (wave == 0) sc_next[j] = (j < n && j != p && sc[j] >= 0.0) ? tot : -1.0;
}

}  // namespace gpmpc
