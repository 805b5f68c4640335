// Pathwise posterior samples (gpmpc_paths_*, gpmpc_rollout_paths; api_paths.inl): S functions drawn once from the posterior
// by Matheron's rule with a random-feature prior (Wilson et al., "Efficiently sampling functions from Gaussian process
// posteriors", ICML 2020), then evaluated per particle.  Per output a and path s, in standardised units:
//     f_{a,s}(z) = m_a(z) + phi_a(z) . w_{a,s} + sum_i v_{a,s,i} k_a(z, x_i),     v_{a,s} = alpha_a - K_a^-1 (Phi_a w_{a,s} + sn_a xi_{a,s})
//     phi_{a,2j}(z) = c_a cos(omega_{a,j} . z), phi_{a,2j+1}(z) = c_a sin(omega_{a,j} . z), c_a = sf_a sqrt(2 / F), omega_{a,j} = eps_{a,j} / ell_a
// Layouts (particles contiguous, so that a wave's loads of one training point's weights or of one feature's weights coalesce):
//     V[Ny][Np][Sld], WT[Ny][Fp][Sld] (w transposed), omega[Ny][F/2][d];  Sld = S rounded up to even, Fp = F rounded up to 16,
//     padded rows / columns are exact zeros.  Phi[Ny][Np][Fp] (K-contiguous A operand of R = Phi W^T + sn xi) is setup scratch.
// Random streams of mc_kernels.hpp's generator (GPMPC_PATHS_STREAM_*): 0x40000000 + a: eps_a (row j, d columns),
// 0x50000000 + a: w_a (row s, F columns), 0x60000000 + a: xi_a (row s, N columns).
// Every kernel is wave64, fp64, without atomics: a result is a function of the data and of PATHS_IB / PATHS_FB only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gpmpc.h"
#include "gp_kernels.hpp"
#include "mc_kernels.hpp"

namespace gpmpc {

constexpr int PATHS_IB = 128;   // training points per block of the evaluation kernel (partial sums per block)
constexpr int PATHS_FB = 16;    // cosine / sine pairs per feature block of the evaluation kernel

// omega[a][j][k] = eps_a[j][k] / ell_a[k]; eps: the caller's [Ny][F/2][d] or the generator.  One thread per (a, j, column pair).
__global__ void __launch_bounds__(256) paths_omega_kernel(const double* __restrict__ hyper, const double* __restrict__ eps,
                                                          unsigned long long seed, double* __restrict__ omega, int Ny, int F2,
                                                          int d) {
    const int kp = (d + 1) / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Ny * F2 * kp) return;
    const int p = (int)(e % kp);
    const long r = e / kp;
    const int j = (int)(r % F2), a = (int)(r / F2);
    const long base = ((long)a * F2 + j) * d;
    double n0, n1;
    if (eps) {
        n0 = eps[base + 2 * p];
        n1 = 2 * p + 1 < d ? eps[base + 2 * p + 1] : 0.0;
    } else {
        mc_normal_pair(seed, (unsigned)GPMPC_PATHS_STREAM_OMEGA + (unsigned)a, (unsigned)j, (unsigned)p, n0, n1);
    }
    const double* hy = hyper + (long)a * (d + 2);
    omega[base + 2 * p] = n0 / hy[2 * p];
    if (2 * p + 1 < d) omega[base + 2 * p + 1] = n1 / hy[2 * p + 1];
}

// WT[a][j][s] = w_a[s][j] for j < F, s < S, zero up to Fp / Sld; w: the caller's [Ny][S][F] or the generator.
// One thread per (a, column pair, s), s fastest (coalesced stores).
__global__ void __launch_bounds__(256) paths_wt_kernel(const double* __restrict__ w, unsigned long long seed,
                                                       double* __restrict__ WT, int Ny, int S, int Sld, int F, int Fp) {
    const int fp2 = Fp / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Ny * fp2 * Sld) return;
    const int s = (int)(e % Sld);
    const long r = e / Sld;
    const int jp = (int)(r % fp2), a = (int)(r / fp2);
    double n0 = 0.0, n1 = 0.0;
    if (s < S && 2 * jp < F) {
        if (w) {
            n0 = w[((long)a * S + s) * F + 2 * jp];
            n1 = w[((long)a * S + s) * F + 2 * jp + 1];
        } else {
            mc_normal_pair(seed, (unsigned)GPMPC_PATHS_STREAM_W + (unsigned)a, (unsigned)s, (unsigned)jp, n0, n1);
        }
    }
    WT[((long)a * Fp + 2 * jp) * Sld + s] = n0;
    WT[((long)a * Fp + 2 * jp + 1) * Sld + s] = n1;
}

// Phi[a][i][2j], [2j + 1] = c_a cos / sin(omega_{a,j} . x_i) for i < n, 2j < F; rows up to `rows` and columns up to Fp are
// zeros.  x_i[k] = X[i * sxi + k * sxk] (the training inputs XT[d][Np], or test points Z[B][d]).
// One thread per (a, i, column pair), pairs fastest.
__global__ void __launch_bounds__(256) paths_phi_kernel(const double* __restrict__ X, long sxi, long sxk,
                                                        const double* __restrict__ omega, const double* __restrict__ hyper,
                                                        double* __restrict__ Phi, int Ny, int n, int rows, int F, int Fp, int d) {
    const int fp2 = Fp / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Ny * rows * fp2) return;
    const int jp = (int)(e % fp2);
    const long r = e / fp2;
    const int i = (int)(r % rows), a = (int)(r / rows);
    double c = 0.0, s = 0.0;
    if (i < n && 2 * jp < F) {
        const double* om = omega + ((long)a * (F / 2) + jp) * d;
        double dot = 0.0;
        for (int k = 0; k < d; ++k) dot = fma(om[k], X[(long)i * sxi + (long)k * sxk], dot);
        sincos(dot, &s, &c);
        const double ca = hyper[(long)a * (d + 2) + d] * sqrt(2.0 / (double)F);
        c *= ca;
        s *= ca;
    }
    double* out = Phi + ((long)a * rows + i) * Fp + 2 * jp;
    out[0] = c;
    out[1] = s;
}

// R[a][i][sc] = sn_a xi_a[c0 + sc][i] for i < N, c0 + sc < S, zero for the other rows < Np: the C operand of
// R = Phi W^T + sn xi (beta = 1) for the path columns [c0, c0 + nc).  xi: the caller's [Ny][S][N] or the generator.
// One thread per (a, row pair, sc), sc fastest.
__global__ void __launch_bounds__(256) paths_xi_kernel(const double* __restrict__ xi, unsigned long long seed,
                                                       const double* __restrict__ hyper, double* __restrict__ R, long ldr,
                                                       long sR, int Ny, int N, int Np, int S, int c0, int nc, int d) {
    const int np2 = Np / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Ny * np2 * nc) return;
    const int sc = (int)(e % nc);
    const long r = e / nc;
    const int ip = (int)(r % np2), a = (int)(r / np2);
    const int s = c0 + sc;
    double n0 = 0.0, n1 = 0.0;
    if (s < S && 2 * ip < N) {
        if (xi) {
            n0 = xi[((long)a * S + s) * N + 2 * ip];
            n1 = 2 * ip + 1 < N ? xi[((long)a * S + s) * N + 2 * ip + 1] : 0.0;
        } else {
            mc_normal_pair(seed, (unsigned)GPMPC_PATHS_STREAM_XI + (unsigned)a, (unsigned)s, (unsigned)ip, n0, n1);
            if (2 * ip + 1 >= N) n1 = 0.0;
        }
    }
    const double sn = hyper[(long)a * (d + 2) + d + 1];
    R[(long)a * sR + (long)(2 * ip) * ldr + sc] = sn * n0;
    R[(long)a * sR + (long)(2 * ip + 1) * ldr + sc] = sn * n1;
}

// V[a][i][c0 + sc] = alpha_a[i] (zero in the padded rows): the C operand of V = alpha - L^-T T1 (alpha = -1, beta = 1).
// One thread per (a, i, sc), sc fastest.
__global__ void __launch_bounds__(256) paths_alpha_fill_kernel(const double* __restrict__ alpha, double* __restrict__ V, long ldv,
                                                               int Ny, int Np, int c0, int nc) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Ny * Np * nc) return;
    const int sc = (int)(e % nc);
    const long r = e / nc;              // a * Np + i
    V[r * ldv + c0 + sc] = alpha[r];
}

// The hot kernel: one thread per path s with its own input z_s in registers; blockIdx.y < nIB is a block of PATHS_IB
// training points -- the block's inputs staged in LDS pre-scaled by 1 / (sqrt 2 ell) as crosscov_kernel does, every thread
// reads the same LDS word (broadcast), the weights V[a][i][s] stream from HBM once, 512 contiguous bytes per wave and i --
//     part[blk][a][s] = sum_{i in block} v_{a,s,i} k_a(z_s, x_i),
// blockIdx.y >= nIB a block of PATHS_FB frequencies,
//     part[blk][a][s] = c_a sum_{j in block} (cos(omega_j . z_s) w_{a,s,2j} + sin(omega_j . z_s) w_{a,s,2j+1}).
// The blocks are fixed by the two constants, not by the grid: paths_finish_kernel adds them in a fixed order.
// grid (ceil(S / 256), nIB + nFB, Ny), 256 threads.
template <int D>
__global__ void __launch_bounds__(256) paths_eval_kernel(const double* __restrict__ XT, const double* __restrict__ hyper,
                                                         const double* __restrict__ V, const double* __restrict__ WT,
                                                         const double* __restrict__ omega, const double* __restrict__ Z,
                                                         double* __restrict__ part, int N, int Np, int S, int Sld, int F, int Fp,
                                                         int nIB) {
    const int tid = threadIdx.x, blk = blockIdx.y, a = blockIdx.z, Ny = gridDim.z;
    const long s = (long)blockIdx.x * 256 + tid;
    const bool live = s < S;
    __shared__ double Xs[PATHS_IB][D], wsc[D], Et[EXPT32_N];
    const double* hy = hyper + (long)a * (D + 2);
    double z[D];
#pragma unroll
    for (int dd = 0; dd < D; ++dd) z[dd] = live ? Z[s * D + dd] : 0.0;
    double acc = 0.0;
    if (blk < nIB) {
        if (tid < D) wsc[tid] = 0.70710678118654752440 / fabs(hy[tid]);
        exp_tab32_fill(Et, tid);
        __syncthreads();
        const int i0 = blk * PATHS_IB, ni = min(PATHS_IB, N - i0);
        for (int e = tid; e < PATHS_IB * D; e += 256) {
            const int dd = e / PATHS_IB, ii = e % PATHS_IB;
            Xs[ii][dd] = ii < ni ? XT[(long)dd * Np + i0 + ii] * wsc[dd] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int dd = 0; dd < D; ++dd) z[dd] *= wsc[dd];
        const double neg_log_sf2 = -log(hy[D] * hy[D]);
        if (live) {
            const double* __restrict__ v = V + ((long)a * Np + i0) * Sld + s;
#pragma unroll 4
            for (int ii = 0; ii < ni; ++ii) {
                double dist = neg_log_sf2;
#pragma unroll
                for (int dd = 0; dd < D; ++dd) {
                    const double df = Xs[ii][dd] - z[dd];
                    dist = fma(df, df, dist);
                }
                acc = fma(exp_tab32_neg(dist, Et), v[(long)ii * Sld], acc);
            }
        }
    } else {
        const int F2 = F / 2, j0 = (blk - nIB) * PATHS_FB, nj = min(PATHS_FB, F2 - j0);
        for (int e = tid; e < nj * D; e += 256) Xs[e / D][e % D] = omega[((long)a * F2 + j0) * D + e];
        __syncthreads();
        if (live) {
            const double* __restrict__ wt = WT + ((long)a * Fp + 2 * j0) * Sld + s;
            for (int jj = 0; jj < nj; ++jj) {
                double dot = 0.0;
#pragma unroll
                for (int dd = 0; dd < D; ++dd) dot = fma(Xs[jj][dd], z[dd], dot);
                double sn, cs;
                sincos(dot, &sn, &cs);
                acc = fma(cs, wt[(long)(2 * jj) * Sld], acc);
                acc = fma(sn, wt[(long)(2 * jj + 1) * Sld], acc);
            }
            acc *= hy[D] * sqrt(2.0 / (double)F);
        }
    }
    if (live) part[((long)blk * Ny + a) * Sld + s] = acc;
}

template <int D>
inline void launch_paths_eval_d(hipStream_t st, const double* XT, const double* hyper, const double* V, const double* WT,
                                const double* omega, const double* Z, double* part, int N, int Np, int S, int Sld, int F, int Fp,
                                int Ny) {
    const int nIB = (N + PATHS_IB - 1) / PATHS_IB, nFB = (F / 2 + PATHS_FB - 1) / PATHS_FB;
    hipLaunchKernelGGL((paths_eval_kernel<D>), dim3((unsigned)((S + 255) / 256), (unsigned)(nIB + nFB), (unsigned)Ny), dim3(256), 0,
                       st, XT, hyper, V, WT, omega, Z, part, N, Np, S, Sld, F, Fp, nIB);
}

inline int paths_part_blocks(int N, int F) { return (N + PATHS_IB - 1) / PATHS_IB + (F / 2 + PATHS_FB - 1) / PATHS_FB; }

inline void launch_paths_eval(hipStream_t st, int d, const double* XT, const double* hyper, const double* V, const double* WT,
                              const double* omega, const double* Z, double* part, int N, int Np, int S, int Sld, int F, int Fp,
                              int Ny) {
#define GPMPC_PE(DD) case DD: launch_paths_eval_d<DD>(st, XT, hyper, V, WT, omega, Z, part, N, Np, S, Sld, F, Fp, Ny); break;
    switch (d) {
        GPMPC_PE(1) GPMPC_PE(2) GPMPC_PE(3) GPMPC_PE(4) GPMPC_PE(5) GPMPC_PE(6) GPMPC_PE(7) GPMPC_PE(8)
        GPMPC_PE(9) GPMPC_PE(10) GPMPC_PE(11) GPMPC_PE(12) GPMPC_PE(13) GPMPC_PE(14) GPMPC_PE(15) GPMPC_PE(16)
        default: break;
    }
#undef GPMPC_PE
}

// Second pass, one thread per path s: f_a = the nblk partial sums of paths_eval_kernel in their fixed order (training-point
// blocks, then feature blocks) + m_a(z_s) when the model adds its prior mean to a prediction (mean_kind != 0).
// Y != Zin only matters to the caller: Y[S][Ny] receives y_s = f_s + noise sn_a eps_s (eps: row s of `stream`, or of the
// caller's eps[S][Ny]; noise == 0 draws nothing), and -- Znext != NULL: a roll-out step that is not the last -- the hand-over
// of mc_step_kernel writes the path's next input z_s = [sa y_s + sb, u] (Znext may be Zin: a thread reads its own row first).
// grid (ceil(S / 256)).
__global__ void __launch_bounds__(MC_BLOCK) paths_finish_kernel(const double* __restrict__ part, int nblk, const double* Zin,
                                                                const double* __restrict__ mpar, int mean_kind,
                                                                const double* __restrict__ hyper, int noise,
                                                                const double* __restrict__ eps, unsigned long long seed,
                                                                unsigned stream, double* __restrict__ Y, double* Znext,
                                                                const double* __restrict__ sa, const double* __restrict__ sb,
                                                                const double* __restrict__ u_next, const double* __restrict__ Kz,
                                                                const double* __restrict__ k0, int S, int Sld, int Ny, int d) {
    const long s = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (s >= S) return;
    double y[DMAX];
    for (int a = 0; a < Ny; ++a) {
        double f = 0.0;
        for (int b = 0; b < nblk; ++b) f += part[((long)b * Ny + a) * Sld + s];
        if (mean_kind) f += mean_eval(mean_kind, mpar + (long)a * MPW, Zin + s * d, 1, d);
        y[a] = f;
    }
    if (noise) {
        for (int a = 0; a < Ny; a += 2) {
            double n0, n1;
            if (eps) {
                n0 = eps[s * Ny + a];
                n1 = a + 1 < Ny ? eps[s * Ny + a + 1] : 0.0;
            } else {
                mc_normal_pair(seed, stream, (unsigned)s, (unsigned)(a >> 1), n0, n1);
            }
            y[a] += hyper[(long)a * (d + 2) + d + 1] * n0;
            if (a + 1 < Ny) y[a + 1] += hyper[(long)(a + 1) * (d + 2) + d + 1] * n1;
        }
    }
    for (int a = 0; a < Ny; ++a) Y[s * Ny + a] = y[a];
    if (!Znext) return;
    const int Nu = d - Ny;
    for (int a = 0; a < Ny; ++a) Znext[s * d + a] = sa[a] * y[a] + sb[a];
    for (int q = 0; q < Nu; ++q) {
        double v;
        if (Kz) {
            v = k0[q];
            for (int c = 0; c < Ny; ++c) v += Kz[q * Ny + c] * y[c];
        } else {
            v = u_next[q];
        }
        Znext[s * d + Ny + q] = v;
    }
}

// gpmpc_paths_eval_grid: f[s][b0 + b][a] = G[a][s][b] + m_a(z_b) for the B points of one chunk (G: [Ny][Sld][ldg], the two
// products Ks^T V + Phi(Z) W^T).  One thread per (s, b, a).
__global__ void __launch_bounds__(256) paths_grid_out_kernel(const double* __restrict__ G, long sG, long ldg,
                                                             const double* __restrict__ Z, const double* __restrict__ mpar,
                                                             int mean_kind, double* __restrict__ f, int S, int B, int b0, int Btot,
                                                             int Ny, int d) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)S * B * Ny) return;
    const int a = (int)(e % Ny), b = (int)((e / Ny) % B);
    const long s = e / ((long)Ny * B);
    double v = G[(long)a * sG + s * ldg + b];
    if (mean_kind) v += mean_eval(mean_kind, mpar + (long)a * MPW, Z + (long)b * d, 1, d);
    f[(s * Btot + b0 + b) * Ny + a] = v;
}

}  // namespace gpmpc
