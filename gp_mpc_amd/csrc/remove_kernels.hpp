// remove_kernels.hpp -- removal of training points from the factors (gpmpc_remove, api_remove.inl).
//
// R = removed indices (n <= REMOVE_W per pass, ascending), S = kept ones in their original order, T = L^-1.  With
//     A = L[S,S] (lower),  E = L[S,R],  TK = T[S,S],  G = T[R,S]
// K[S,S] = [A E][A E]^T, so L' = chol(K[S,S]) is what an orthogonal Q leaves of [A E] Q = [L' 0], and L'^-1 is the
// leading block of Q^T [TK; G].  Q is a product of one Householder reflector per kept column i, in increasing order,
//     H_i = I - tau_i [1; v_i][1; v_i]^T     on coordinate i and the n removed coordinates,
// chosen so that [A[i,i], E[i,:]] H_i = [+rho_i, 0], rho_i = sqrt(A[i,i]^2 + |E[i,:]|^2).  With
// delta = |e|^2 / (a + rho) = rho - a (free of cancellation):  v = -e / delta,  tau = delta / rho,  new diagonal a + delta.
// |e|^2 == 0: tau = 0, nothing to do -- every column below the first removed index, and all of them for trailing removals.
// Both applications are one recurrence on independent items (an n-vector x and one scalar s_i per reflector):
//     t = s_i + v_i . x;   s_i -= tau_i t;   x -= tau_i t v_i
//   L:  items = rows r below the panel,           x = E[r,:],  s_i = A[r, 64p+i]     (column 64p+i of L')
//   T:  items = columns c up to the panel's end,  x = G[:,c],  s_i = TK[64p+i, c]    (row 64p+i of L'^-1)
// Structural zeros stay exact: the support of v_i is the removed columns r < s_i, and whatever could fill an entry above
// the diagonal is a sum of products 0 * x.
//
// Launches: one gather (compacts L and T into the new workspace, fills E and G), then per 64-column panel at or above the
// first removed index a panel kernel (generates the 64 reflectors in order on the panel's own rows, leaves V and tau in
// memory) and an apply kernel (all other items, no synchronisation between them).  Stream order is the only ordering
// between launches; no workgroup waits for another one.
// E and G are stored transposed / as they lie: Et[a][k][Np], G[a][k][Np] (k < NX), so that lanes that own consecutive items
// read consecutive addresses.  NX (4, 16 or 64) is the register width of an item's x; rows k >= n of Et / G are zero.
#pragma once
#include <hip/hip_runtime.h>

namespace gpmpc {

constexpr int REMOVE_W = 64;        // removed points per pass

// grid (Np1 + 2 NX, Np1 / 256 rounded up, Ny).  src[i]: old index of new index i (-1: padding), rem[k]: old index of the
// k-th removed point (k < n).  Rows y < Np1: row y of L1 and T1 (lower part from the old factors, identity in the padding;
// above the diagonal zeros, written only if zero_upper -- a fresh workspace is cleared already); then NX rows of Et, NX of G.
__global__ void __launch_bounds__(256) remove_gather_kernel(const double* __restrict__ L0, const double* __restrict__ T0,
                                                            int Np0, double* __restrict__ L1, double* __restrict__ T1, int Np1,
                                                            double* __restrict__ Et, double* __restrict__ G,
                                                            const int* __restrict__ src, const int* __restrict__ rem, int n,
                                                            int NX, int zero_upper) {
    const int j = (int)blockIdx.y * 256 + (int)threadIdx.x, y = blockIdx.x, a = blockIdx.z;
    if (j >= Np1) return;
    const double* l0 = L0 + (long)a * Np0 * Np0;
    const double* t0 = T0 + (long)a * Np0 * Np0;
    const int sj = src[j];
    if (y < Np1) {
        const int i = y;
        if ((int)blockIdx.y * 256 > i && !zero_upper) return;
        const long o = ((long)a * Np1 + i) * Np1 + j;
        const int si = src[i];
        double lv = 0.0, tv = 0.0;
        if (j <= i) {
            if (si >= 0) {                                   // (sj >= 0 as well: the padding follows the points)
                lv = l0[(long)si * Np0 + sj];
                tv = t0[(long)si * Np0 + sj];
            } else if (i == j) {
                lv = tv = 1.0;
            }
        }
        L1[o] = lv;
        T1[o] = tv;
        return;
    }
    const int k = (y - Np1) % NX;
    const bool isG = y - Np1 >= NX;
    const long o = ((long)a * NX + k) * Np1 + j;
    double v = 0.0;
    if (k < n && sj >= 0) {
        const int r = rem[k];
        if (!isG && r < sj) v = l0[(long)sj * Np0 + r];      // E[j][k] = L[s_j][r_k]
        if (isG && sj < r) v = t0[(long)r * Np0 + sj];       // G[k][j] = T[r_k][s_j]
    }
    (isG ? G : Et)[o] = v;
}

// Panel p: grid (Ny), 256 threads.  Thread (r = tid & 63, q = tid >> 6) owns row 64p + r and the NX / 4 removed
// coordinates k = q NX/4 ..; the partial dot products of the four q are added in a fixed order.
template <int NX>
__global__ void __launch_bounds__(256) remove_panel_kernel(double* __restrict__ L1, const double* __restrict__ Et, int Np1,
                                                           int p, double* __restrict__ V, double* __restrict__ tau) {
    constexpr int KQ = NX / 4;
    const int tid = threadIdx.x, r = tid & 63, q = tid >> 6, a = blockIdx.x;
    __shared__ double At[64][65];       // At[c][r] = A[64p + r][64p + c]
    __shared__ double Es[NX][64];       // Es[k][r] = E[64p + r][k]
    __shared__ double red[4][64];
    double* l1 = L1 + (long)a * Np1 * Np1 + (long)64 * p * Np1 + 64 * p;
    const double* et = Et + (long)a * NX * Np1 + 64 * p;
    double* vg = V + (long)a * 64 * NX;
    for (int e = tid; e < 4096; e += 256) At[e & 63][e >> 6] = l1[(long)(e >> 6) * Np1 + (e & 63)];
    for (int e = tid; e < 64 * NX; e += 256) Es[e >> 6][e & 63] = et[(long)(e >> 6) * Np1 + (e & 63)];
    __syncthreads();
    for (int i = 0; i < 64; ++i) {
        double nrm = 0.0;               // every thread forms |e|^2 in the same order: the same bits, a uniform branch
#pragma unroll
        for (int k = 0; k < NX; ++k) nrm = fma(Es[k][i], Es[k][i], nrm);
        if (!(nrm > 1e-280)) {          // (below that 1 / delta overflows; such a row is zero to every digit of a)
            if (r == i) {
                for (int k = q * KQ; k < (q + 1) * KQ; ++k) vg[i * NX + k] = 0.0;
                if (q == 0) tau[a * 64 + i] = 0.0;
            }
            continue;
        }
        const double aii = At[i][i], air = At[i][r];      // (read before the barrier: q = 0 overwrites A[r][i] behind it)
        const double rho = sqrt(fma(aii, aii, nrm));
        const double delta = nrm / (aii + rho);
        const double tu = delta / rho, ninv = -1.0 / delta;
        double v[KQ];
        double part = 0.0;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            v[k] = Es[q * KQ + k][i] * ninv;
            part = fma(v[k], Es[q * KQ + k][r], part);
        }
        red[q][r] = part;
        if (r == i) {
#pragma unroll
            for (int k = 0; k < KQ; ++k) vg[i * NX + q * KQ + k] = v[k];
            if (q == 0) tau[a * 64 + i] = tu;
        }
        __syncthreads();
        if (r > i) {
            const double t = air + ((red[0][r] + red[1][r]) + (red[2][r] + red[3][r]));
            const double tt = tu * t;
#pragma unroll
            for (int k = 0; k < KQ; ++k) Es[q * KQ + k][r] = fma(-tt, v[k], Es[q * KQ + k][r]);
            if (q == 0) At[i][r] = air - tt;
        } else if (r == i && q == 0) {
            At[i][i] = aii + delta;     // = rho
        }
        __syncthreads();
    }
    for (int e = tid; e < 4096; e += 256)
        if ((e & 63) <= (e >> 6)) l1[(long)(e >> 6) * Np1 + (e & 63)] = At[e & 63][e >> 6];
}

// Panel p applied to every other item: grid ((nT + nL) / 64 rounded up, Ny), 64 threads, one item per lane.
// Items 0 .. nT-1: columns c of T' (nT = min(64 (p + 1), N1)); then nL = N1 - 64 (p + 1) rows of L' below the panel.
template <int NX>
__global__ void __launch_bounds__(64) remove_apply_kernel(double* __restrict__ L1, double* __restrict__ T1,
                                                          double* __restrict__ Et, double* __restrict__ G, int Np1, int N1,
                                                          int p, const double* __restrict__ V, const double* __restrict__ tau) {
    const int lane = threadIdx.x, a = blockIdx.y;
    __shared__ double Vs[64][NX];
    __shared__ double ts[64];
    const double* vg = V + (long)a * 64 * NX;
    for (int e = lane; e < 64 * NX; e += 64) Vs[e / NX][e % NX] = vg[e];
    ts[lane] = tau[a * 64 + lane];
    __syncthreads();
    const int nT = min(64 * (p + 1), N1), nL = max(N1 - 64 * (p + 1), 0);
    const int item = (int)blockIdx.x * 64 + lane;
    if (item >= nT + nL) return;
    double* xp;
    double* sp;
    long ss;
    if (item < nT) {
        xp = G + (long)a * NX * Np1 + item;
        sp = T1 + (long)a * Np1 * Np1 + (long)64 * p * Np1 + item;
        ss = Np1;
    } else {
        const int row = 64 * (p + 1) + (item - nT);
        xp = Et + (long)a * NX * Np1 + row;
        sp = L1 + (long)a * Np1 * Np1 + (long)row * Np1 + 64 * p;
        ss = 1;
    }
    double x[NX];
#pragma unroll
    for (int k = 0; k < NX; ++k) x[k] = xp[(long)k * Np1];
    for (int i = 0; i < 64; ++i) {
        const double tu = ts[i];
        if (tu == 0.0) continue;
        const double s = sp[i * ss];
        double t0 = s, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
        for (int k = 0; k < NX; k += 4) {
            t0 = fma(Vs[i][k], x[k], t0);
            t1 = fma(Vs[i][k + 1], x[k + 1], t1);
            t2 = fma(Vs[i][k + 2], x[k + 2], t2);
            t3 = fma(Vs[i][k + 3], x[k + 3], t3);
        }
        const double tt = tu * ((t0 + t1) + (t2 + t3));
        sp[i * ss] = s - tt;
#pragma unroll
        for (int k = 0; k < NX; ++k) x[k] = fma(-tt, Vs[i][k], x[k]);
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) xp[(long)k * Np1] = x[k];
}

}  // namespace gpmpc
