// fitc_kernels.hpp -- the N-sized work of the FITC sparse model (gpmpc_sparse_fitc, api_sparse.inl).
//
// Per output a with (ell, sf, sn), inducing points Xu (M of them) and Luu = chol(k(Xu, Xu) + 1e-6 sf^2 I):
//     V = Luu^-1 k(Xu, X)  [M x N],   lambda_i = max(sf^2 - sum_m V_mi^2, 0) + sn^2,
//     Vs = V Lambda^-1/2,   B = I + Vs Vs^T,   r = Vs Lambda^-1/2 y.
// The training points are visited in chunks; the chunk's V comes from the launches of gpmpc_covar (cross-covariances, one
// product with Luu^-1) as VT[a][c][Mp] -- one ROW per training point c of the chunk, the inducing index contiguous.  Here:
//   fitc_gather_kernel   the chunk's training inputs as rows (the handle keeps X transposed)
//   fitc_scale_kernel    per row: q, lambda, the scaling by lambda^-1/2 in place, ys = y lambda^-1/2; rows beyond the chunk's
//                        count and columns beyond M become exact zeros, so the padding of B stays the identity
//   fitc_syrk_kernel     B += Vs Vs^T on the lower 64 x 64 tiles (fp64 MFMA, LDS-staged operands), accumulated in place over
//                        the chunks; the diagonal tiles add r += Vs ys from the operand they have staged anyway
//   fitc_eye_kernel      B = I before the first chunk
//   fitc_cmat_kernel     C = I - B^-1 (identity in the padding, so that what is factored from it keeps an identity padding)
//   fitc_symavg_kernel   P = (P + P^T) / 2 in place: P = Luu^-T C Luu^-1 comes out of two products with rounding errors that are
//                        not symmetric, and the quadratic forms k P k^T (entries of P ~ 1 / jitter, results ~ sf^2) keep their
//                        digits only if BOTH triangles enter -- mirroring one triangle costs a digit (measured: 6e-12 against
//                        6e-13 sf^2 at N = M = 130, sn = 0.1)
//   fitc_revt_kernel     out[i][j] = in[n-1-j][n-1-i]: turns the Cholesky factor of the index-reversed C into the LOWER
//                        triangular S with S^T S = C (and its inverse into S^-1); W = S Luu^-1 is then lower triangular with
//                        W^T W = P
// Stream order is the only synchronisation: every launch owns what it writes, no workgroup waits for another one.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_kernels.hpp"
#include "mfma_f64.hpp"

namespace gpmpc {

// Z[c][k] = XT[k][c0 + c] for c < nc.  grid (nc * d / 256 rounded up).
__global__ void __launch_bounds__(256) fitc_gather_kernel(const double* __restrict__ XT, double* __restrict__ Z, int NpS,
                                                          int c0, int nc, int d) {
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (g >= nc * d) return;
    const int c = g / d, k = g % d;
    Z[g] = XT[(long)k * NpS + c0 + c];
}

// B[a] = I.  grid (Mp * Mp / 256, Ny).
__global__ void __launch_bounds__(256) fitc_eye_kernel(double* __restrict__ Bm, int Mp) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(g / Mp), j = (int)(g % Mp);
    Bm[(long)blockIdx.y * Mp * Mp + g] = i == j ? 1.0 : 0.0;
}

// One wave per row c of the chunk.  grid (Bp / 4, Ny), 256 threads.  hyper: the model's own rows [ell.., sf, sn] (the
// factor behind V was built with the inducing jitter in place of sn).  Y: the source's targets [Ny][NpS].
__global__ void __launch_bounds__(256) fitc_scale_kernel(double* __restrict__ VT, const double* __restrict__ Y,
                                                         const double* __restrict__ hyper, double* __restrict__ ys, int c0,
                                                         int nc, int Bp, int M, int Mp, int NpS, int d) {
    const int lane = threadIdx.x & 63, c = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), a = blockIdx.y;
    double* __restrict__ row = VT + ((long)a * Bp + c) * Mp;
    if (c >= nc) {
        for (int m = lane; m < Mp; m += 64) row[m] = 0.0;
        if (lane == 0) ys[(long)a * Bp + c] = 0.0;
        return;
    }
    double q = 0.0;
    for (int m = lane; m < M; m += 64) q = fma(row[m], row[m], q);
    q = wave_sum(q);
    const double sf = hyper[(long)a * (d + 2) + d], sn = hyper[(long)a * (d + 2) + d + 1];
    const double lam = fmax(sf * sf - q, 0.0) + sn * sn;
    const double sc = 1.0 / sqrt(lam);
    for (int m = lane; m < Mp; m += 64) row[m] = m < M ? row[m] * sc : 0.0;
    if (lane == 0) ys[(long)a * Bp + c] = Y[(long)a * NpS + c0 + c] * sc;
}

constexpr int FITC_KS = 16;     // training points per staged slab
constexpr int FITC_LDP = 80;    // LDS row length in doubles: 64 + 16, so that the k rows l >> 4 and (l >> 4) + 1 of a fragment
                                // read (lanes l and l + 16 of one 32-lane half) fall into opposite halves of the 256-byte bank row

// B[a][m][n] += sum_c VT[a][c][m] VT[a][c][n] for the lower tiles (tm >= tn) and, by the diagonal tiles,
// r[a][m] += sum_c VT[a][c][m] ys[a][c].  grid (T (T + 1) / 2, Ny) with T = Mp / 64, 256 threads: four waves in 2 x 2, each
// a 32 x 32 quarter of the tile as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 (A[i][k] = Vs[k][m0 + i], B[k][j] = Vs[k][n0 + j]:
// both fragments are rows of the staged slab).  The next slab's global loads are in flight while the current one is multiplied.
// Bp % 16 == 0, Mp % 64 == 0; every element of the chunk is read, the padding holds zeros (fitc_scale_kernel).
__global__ void __launch_bounds__(256) fitc_syrk_kernel(const double* __restrict__ VT, const double* __restrict__ ys,
                                                        double* __restrict__ Bm, double* __restrict__ r, int Bp, int Mp,
                                                        int crow_mode) {
    __shared__ double As[FITC_KS][FITC_LDP];
    __shared__ double Bs[FITC_KS][FITC_LDP];
    __shared__ double ysS[FITC_KS];
    __shared__ double red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = blockIdx.y;
    int tm = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);      // blockIdx.x = tm (tm + 1) / 2 + tn
    while ((tm + 1) * (tm + 2) / 2 <= (int)blockIdx.x) ++tm;
    while (tm * (tm + 1) / 2 > (int)blockIdx.x) --tm;
    const int tn = (int)blockIdx.x - tm * (tm + 1) / 2;
    const int m0 = tm * 64, n0 = tn * 64;
    const bool diag = tm == tn;
    const double* __restrict__ Va = VT + (long)a * Bp * Mp;
    const double* __restrict__ ya = ys + (long)a * Bp;
    const int wm = 32 * (wave >> 1), wn = 32 * (wave & 1), li = lane & 15, lk = lane >> 4;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    double racc = 0.0;
    double pa[4], pb[4], py = 0.0;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, k = idx >> 6, col = idx & 63;
            pa[q] = Va[(long)(k0 + k) * Mp + m0 + col];
            if (!diag) pb[q] = Va[(long)(k0 + k) * Mp + n0 + col];
        }
        if (diag && tid < FITC_KS) py = ya[k0 + tid];
    };
    fetch(0);
    for (int k0 = 0; k0 < Bp; k0 += FITC_KS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, k = idx >> 6, col = idx & 63;
            As[k][col] = pa[q];
            Bs[k][col] = diag ? pa[q] : pb[q];
        }
        if (diag && tid < FITC_KS) ysS[tid] = py;
        __syncthreads();
        if (k0 + FITC_KS < Bp) fetch(k0 + FITC_KS);
#pragma unroll
        for (int kk = 0; kk < FITC_KS / 4; ++kk) {
            const int k = 4 * kk + lk;
            const double a0 = As[k][wm + li], a1 = As[k][wm + 16 + li];
            const double b0 = Bs[k][wn + li], b1 = Bs[k][wn + 16 + li];
            acc[0][0] = mfma16(a0, b0, acc[0][0]);
            acc[0][1] = mfma16(a0, b1, acc[0][1]);
            acc[1][0] = mfma16(a1, b0, acc[1][0]);
            acc[1][1] = mfma16(a1, b1, acc[1][1]);
        }
        if (diag) {
#pragma unroll
            for (int k = 0; k < 4; ++k) racc = fma(As[4 * wave + k][lane], ysS[4 * wave + k], racc);
        }
        __syncthreads();
    }
    double* __restrict__ Ba = Bm + (long)a * Mp * Mp;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int m = m0 + wm + 16 * i + crow(lane, rr, crow_mode), n = n0 + wn + 16 * j + li;
                Ba[(long)m * Mp + n] += acc[i][j][rr];
            }
    if (diag) {
        red[wave][lane] = racc;
        __syncthreads();
        if (wave == 0) r[(long)a * Mp + m0 + lane] += (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    }
}

// In place: C = I - Binv on the leading M x M block, the identity in the padding.  grid (Mp * Mp / 256, Ny).
__global__ void __launch_bounds__(256) fitc_cmat_kernel(double* __restrict__ Binv, int M, int Mp) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(g / Mp), j = (int)(g % Mp);
    double* p = Binv + (long)blockIdx.y * Mp * Mp + g;
    const double e = i == j ? 1.0 : 0.0;
    *p = (i < M && j < M) ? e - *p : e;
}

// A = (A + A^T) / 2 in place, n % 64 == 0.  grid (n / 64, n / 64, Ny); the workgroup of tile (tm, tn), tn <= tm, owns that tile
// and its mirror image, the others leave at once.  Both images get the same bits (the sum commutes).
__global__ void __launch_bounds__(256) fitc_symavg_kernel(double* __restrict__ A, int n) {
    const int tn = blockIdx.x, tm = blockIdx.y, tid = threadIdx.x;
    if (tn > tm) return;
    __shared__ double lo[64][65];
    __shared__ double up[64][65];
    double* __restrict__ Aa = A + (long)blockIdx.z * n * n;
    const int m0 = tm * 64, n0 = tn * 64;
    for (int idx = tid; idx < 4096; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        lo[r][c] = Aa[(long)(m0 + r) * n + n0 + c];
        up[r][c] = Aa[(long)(n0 + r) * n + m0 + c];
    }
    __syncthreads();
    for (int idx = tid; idx < 4096; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        Aa[(long)(m0 + r) * n + n0 + c] = 0.5 * (lo[r][c] + up[c][r]);
        if (tm != tn) Aa[(long)(n0 + r) * n + m0 + c] = 0.5 * (up[r][c] + lo[c][r]);
    }
}

// out[a][i][j] = in[a][n-1-j][n-1-i] (rev != 0) or in[a][j][i] (rev == 0) for n x n matrices, n % 64 == 0, through a 64 x 64
// LDS tile so that both sides are accessed along rows; `shift` is added to the diagonal entries that belong to the leading
// M x M block of `in` (the padding keeps its exact identity).  grid (n / 64, n / 64, Ny), 256 threads.
__global__ void __launch_bounds__(256) fitc_revt_kernel(const double* __restrict__ in, double* __restrict__ out, int n, int rev,
                                                        double shift, int M) {
    __shared__ double tile[64][65];
    const int i0 = (int)blockIdx.y * 64, j0 = (int)blockIdx.x * 64, tid = threadIdx.x;
    const double* __restrict__ ia = in + (long)blockIdx.z * n * n;
    double* __restrict__ oa = out + (long)blockIdx.z * n * n;
    const int rowbase = rev ? n - 64 - j0 : j0, colbase = rev ? n - 64 - i0 : i0;
    for (int idx = tid; idx < 4096; idx += 256) {
        const int rr = idx >> 6, c = idx & 63;
        tile[rr][c] = ia[(long)(rowbase + rr) * n + colbase + c];
    }
    __syncthreads();
    for (int idx = tid; idx < 4096; idx += 256) {
        const int rr = idx >> 6, c = idx & 63, i = i0 + rr, j = j0 + c;
        const double v = rev ? tile[63 - c][63 - rr] : tile[c][rr];
        const int src = rev ? n - 1 - i : i;
        oa[(long)i * n + j] = (i == j && src < M) ? v + shift : v;
    }
}

}  // namespace gpmpc
