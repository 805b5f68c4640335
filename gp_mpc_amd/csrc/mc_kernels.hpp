// Monte Carlo roll-outs (gpmpc_rollout_mc, api_mc.inl): a counter-based normal generator, the hand-over between two time
// steps of S particles, and a deterministic moment reduction.  The prediction itself is predict_chunk's, unchanged.
//
// Generator: Philox-4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).
// key = (seed low word, seed high word), counter = (row, column pair, stream, 0).  One call gives four words w0..w3, i.e. two
// 53-bit uniforms in (0, 1], u1 from (w0, w1) and u2 from (w2, w3): ((hi >> 5) * 2^26 + (lo >> 6) + 1) * 2^-53, and Box-Muller
// turns them into the standard normals of columns 2j (r cos 2 pi u2) and 2j + 1 (r sin 2 pi u2), r = sqrt(-2 log u1).
// The value at (seed, stream, row, column) is a function of those four numbers only: not of the launch geometry, of the
// number of rows, or of how the particles are chunked.  Streams: 0 = the initial particles, 1 + t = the draw of time step t.
// The 32 x 32 -> 64 products are written as uint64_t products: the emulated build compiles the same text.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gp_kernels.hpp"

namespace gpmpc {

constexpr int MC_BLOCK = 256;       // particles per workgroup, and per partial sum of the moment reduction

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the two standard normals of (row, column pair `pair`): columns 2 pair and 2 pair + 1
__device__ inline void mc_normal_pair(unsigned long long seed, unsigned stream, unsigned row, unsigned pair, double& n0, double& n1) {
    uint32_t w[4];
    philox4x32_10(row, pair, stream, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), w);
    const double u1 = (double)((((uint64_t)(w[0] >> 5)) << 26) + (uint64_t)(w[1] >> 6) + 1ull) * 0x1p-53;
    const double u2 = (double)((((uint64_t)(w[2] >> 5)) << 26) + (uint64_t)(w[3] >> 6) + 1ull) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    n0 = r * cos(ang);
    n1 = r * sin(ang);
}

// out[rows][cols] = the normals of (seed, stream): one thread per (row, column pair).  grid (ceil(rows * pairs / 256)).
__global__ void __launch_bounds__(MC_BLOCK) mc_randn_kernel(unsigned long long seed, unsigned stream, int rows, int cols,
                                                            double* __restrict__ out) {
    const int pairs = (cols + 1) / 2;
    const long e = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (e >= (long)rows * pairs) return;
    const long row = e / pairs;
    const int j = (int)(e % pairs);
    double n0, n1;
    mc_normal_pair(seed, stream, (unsigned)row, (unsigned)j, n0, n1);
    out[row * cols + 2 * j] = n0;
    if (2 * j + 1 < cols) out[row * cols + 2 * j + 1] = n1;
}

// Particle s: z_s = z0 + L0 eps0_s, L0[d][d] lower triangular, eps0_s = row s of stream 0 (or of the caller's eps0[S][d]).
// One thread per particle.  grid (ceil(S / 256)).
__global__ void __launch_bounds__(MC_BLOCK) mc_init_kernel(const double* __restrict__ z0, const double* __restrict__ L0,
                                                           const double* __restrict__ eps0, unsigned long long seed,
                                                           double* __restrict__ Z, int S, int d) {
    const long s = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (s >= S) return;
    double e[DMAX];
    for (int j = 0; j < d; j += 2) {
        double n0, n1;
        if (eps0) {
            n0 = eps0[s * d + j];
            n1 = j + 1 < d ? eps0[s * d + j + 1] : 0.0;
        } else {
            mc_normal_pair(seed, 0u, (unsigned)s, (unsigned)(j >> 1), n0, n1);
        }
        e[j] = n0;
        if (j + 1 < d) e[j + 1] = n1;
    }
    for (int k = 0; k < d; ++k) {
        double v = z0[k];
        for (int j = 0; j <= k; ++j) v += L0[k * d + j] * e[j];
        Z[s * d + k] = v;
    }
}

// The hand-over of time step t, one thread per particle: from (mean_s, var_s) = the prediction at the particle's input
//   y_s = mean_s + sqrt(max(var_s, 0) + noise sn_a^2) eps_{t,s}      (eps: row s of `stream`, or of the caller's eps[S][Ny])
// is drawn, written to Y[S][Ny] (the particle record of the step, or scratch), and -- Z != NULL: every step but the last --
// the particle's next input z_s = [sa y_s + sb, u] with u = u_next (open loop: the same control for every particle) or
// u = Kz y_s + k0 (Kz != NULL: state feedback per particle, rollout_feed_kernel's convention).  sn: hyper rows [d + 2].
// grid (ceil(S / 256)).
__global__ void __launch_bounds__(MC_BLOCK) mc_step_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                           const double* __restrict__ hyper, int noise,
                                                           const double* __restrict__ eps, unsigned long long seed,
                                                           unsigned stream, double* __restrict__ Y, double* __restrict__ Z,
                                                           const double* __restrict__ sa, const double* __restrict__ sb,
                                                           const double* __restrict__ u_next, const double* __restrict__ Kz,
                                                           const double* __restrict__ k0, int S, int Ny, int d) {
    const long s = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (s >= S) return;
    double y[DMAX];
    for (int a = 0; a < Ny; a += 2) {
        double n0, n1;
        if (eps) {
            n0 = eps[s * Ny + a];
            n1 = a + 1 < Ny ? eps[s * Ny + a + 1] : 0.0;
        } else {
            mc_normal_pair(seed, stream, (unsigned)s, (unsigned)(a >> 1), n0, n1);
        }
        for (int q = 0; q < 2 && a + q < Ny; ++q) {
            const int b = a + q;
            const double sn = hyper[(long)b * (d + 2) + d + 1];
            const double sd = sqrt(fmax(var[s * Ny + b], 0.0) + (noise ? sn * sn : 0.0));
            const double v = mean[s * Ny + b] + sd * (q ? n1 : n0);
            y[b] = v;
            Y[s * Ny + b] = v;
        }
    }
    if (!Z) return;
    const int Nu = d - Ny;
    for (int a = 0; a < Ny; ++a) Z[s * d + a] = sa[a] * y[a] + sb[a];
    for (int q = 0; q < Nu; ++q) {
        double v;
        if (Kz) {
            v = k0[q];
            for (int c = 0; c < Ny; ++c) v += Kz[q * Ny + c] * y[c];
        } else {
            v = u_next[q];
        }
        Z[s * d + Ny + q] = v;
    }
}

// ---- moments of the S vectors y_s: two passes, partial sums over fixed blocks of 256 particles, combined in a fixed order.
// No atomics: the result is a function of the data (and S) only.
// Pass over the particles.  center == NULL: part[blk][a] = sum of y_a over the block's particles (n = Ny quantities);
// center[Ny] given: part[blk][p] = sum of (y_a - center_a)(y_b - center_b), p = a (a + 1) / 2 + b, b <= a (n = Ny (Ny + 1) / 2).
// grid (ceil(S / 256)), 256 threads; every thread takes part in every reduction (no early exit).
__global__ void __launch_bounds__(MC_BLOCK) mc_moments_partial_kernel(const double* __restrict__ Y, const double* __restrict__ center,
                                                                      double* __restrict__ part, int S, int Ny) {
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x * MC_BLOCK + tid;
    const bool live = s < S;
    __shared__ double red[4];
    double y[DMAX];
    for (int a = 0; a < Ny; ++a) y[a] = live ? Y[s * Ny + a] - (center ? center[a] : 0.0) : 0.0;
    const int n = center ? Ny * (Ny + 1) / 2 : Ny;
    int a = 0, b = 0;
    for (int p = 0; p < n; ++p) {
        double v = center ? y[a] * y[b] : y[p];
        v = wave_sum(v);
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) part[(long)blockIdx.x * n + p] = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
        if (++b > a) { ++a; b = 0; }
    }
}

// Quantity p = blockIdx.x of n: the nblk partial sums in a fixed order (thread i: blocks i, i + 256, ...; then the wave and
// workgroup sums), times `scale`.  sym == 0: out[p] (the mean, scale = 1 / S); sym != 0: p = (a, b) of the lower triangle,
// out[a][b] = out[b][a] (the covariance, scale = 1 / (S - 1), or 0 for S = 1).  grid (n), 256 threads.
__global__ void __launch_bounds__(MC_BLOCK) mc_moments_final_kernel(const double* __restrict__ part, int nblk, int n, double scale,
                                                                    double* __restrict__ out, int sym, int Ny) {
    const int tid = threadIdx.x, p = blockIdx.x;
    __shared__ double red[4];
    double v = 0.0;
    for (int i = tid; i < nblk; i += MC_BLOCK) v += part[(long)i * n + p];
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const double r = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
        if (!sym) {
            out[p] = r;
        } else {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= p) ++a;
            const int b = p - a * (a + 1) / 2;
            out[a * Ny + b] = r;
            out[b * Ny + a] = r;
        }
    }
}

}  // namespace gpmpc
