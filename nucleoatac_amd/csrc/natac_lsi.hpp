// natac_lsi.hpp -- the kernels behind `pyatac cluster` (this package's own command: the reference has no such tool): the truncated SVD of
// the weighted cell-by-window matrix by randomized subspace iteration (natac_sparse_lsi, include/natac.h), fp64 throughout.
//
// The matrix arrives as natac_region_cell_counts leaves it: CSR with one row per window, the cells ascending within a row.  X is its
// transpose, cells x windows (n x m), with the entry of count a in window w and cell c weighted to
//   t = a' * col_scale[c] * row_weight[w]   (a' = 1 with binarize, else a),   X[c, w] = t   or   log1p(t * scale).
// The algorithm, with orth(B) the orthonormalisation of the columns of a tall block:
//   1. Q = orth(q0)                                                      (m x r; rows of dropped windows are zeroed first)
//   2. n_iter times:  Y = orth(X Q)   (n x r),   Q = orth(X^T Y)   (m x r)
//   3. Y = X Q,  G = Y^T Y = W diag(lam) W^T with lam descending          (r x r, cyclic Jacobi on the host)
//   4. sigma = sqrt(lam),  U = Y W / sigma,  V = Q W
// orth is CholeskyQR2: G = B^T B on the device, G = R^T R on the host (plain C++, r <= 64), B <- B R^-1 on the device (a forward
// substitution per row), and all of that once more.  A pivot of at most r * eps * max(diag G) means the block has lost rank: status 1.
// Every step scales with the operands and every threshold is relative, so a power of two in row_weight, col_scale or q0 changes no bit
// of U and V -- as long as the Gram matrices stay inside fp64.  One that does not (an entry not finite; max(diag G) so small that the
// pivot floor r * eps * max(diag G) is below DBL_MIN, where the pivots sit among the denormals and lose bits without falling under the
// floor; a block of non-zero entries whose squares all vanished) ends the call with status 2.
//
// Kernels:
//   lsi_weight / lsi_transpose   one pass over the entries: the weighted values in window order, and the same values with their window
//                   indices in cell order.  The order of the second copy -- for every cell its windows ascending -- is a stable counting
//                   sort by cell, and it runs on the HOST: it moves integers only (the permutation and every entry's window), the
//                   device applies it to the fp64 values, which the host never sees.
//   lsi_spmm_*      out[i, :] = sum over the entries e of row i of val[e] * B[idx[e], :], for both products (the window-order copy gives
//                   X^T Y, the cell-order copy X Q).  r is padded to RP = 16, 32 or 64; a wave is 64 / RP lane groups, lane j of a group
//                   owns column j and loads B[idx * r + j] coalesced.  Rows go by their length L:
//                     L <= LSI_SHORT_MAX   every lane group takes a row of its own, its entries in order;
//                     L <= LSI_WAVE_MAX    one wave per row, group g takes the entries g, g + G, ...; the groups' sums are combined
//                                          by a butterfly of fixed shape;
//                     longer               one workgroup per row, wave w's group g takes the entries 4 w G + g ..., the four waves'
//                                          sums are added in wave order through LDS.
//                   With RP = 64 a wave is one group and the first two arms do the same work.
//   lsi_gram_slab / lsi_gram_sum   B^T B of a tall block: a workgroup keeps the RP x RP partial of a slab of LSI_SLAB rows in
//                   registers (a 16 x 16 grid of threads, (RP / 16)^2 sums each, rows in order) and writes it out; the partials are
//                   added in slab order.
//   lsi_rows_small  B <- B R^-1 (forward substitution) or B <- B M / d: one row per thread, the row in registers, R or M read through
//                   the scalar cache; rows go in and out through LDS so that global accesses stay coalesced.
//   lsi_any_nonzero whether a block holds anything but zeros: asked only when a Gram diagonal is zero, to tell an empty block (status 1)
//                   from one whose squares vanished (status 2).
// Every sum has a fixed shape -- a row's entries, the groups, the waves, a slab's rows, the slabs -- and there are no floating-point
// atomics: the result is a pure function of the operands.
// Behind the kernels: the host's Cholesky and Jacobi, and the entry point.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace natac_lsi {

constexpr int LSI_BLOCK = 256;              // 4 waves
constexpr int LSI_MAX_R = 64;               // NATAC_LSI_MAX_R: one column per lane
constexpr int LSI_SHORT_MAX = 32;           // NATAC_LSI_SHORT_MAX
constexpr int LSI_WAVE_MAX = 4096;          // NATAC_LSI_WAVE_MAX
constexpr int LSI_SLAB = 1024;              // rows per workgroup of the Gram kernel
constexpr int LSI_CHUNK = 32;               // rows of a slab in LDS at a time
constexpr int LSI_ROWS = 64;                // rows per workgroup (one wave) of lsi_rows_small

// val[e] of every entry in window order; erow[e] is the entry's window
__global__ void __launch_bounds__(LSI_BLOCK) lsi_weight(const int *__restrict__ col, const int *__restrict__ count, const int *__restrict__ erow,
                                                        long long nnz, const double *__restrict__ row_weight,
                                                        const double *__restrict__ col_scale, double scale, int transform, int binarize,
                                                        double *__restrict__ val) {
    for (long long e = (long long)blockIdx.x * LSI_BLOCK + threadIdx.x; e < nnz; e += (long long)gridDim.x * LSI_BLOCK) {
        const double a = binarize ? 1.0 : (double)count[e];
        const double t = a * col_scale[col[e]] * row_weight[erow[e]];
        val[e] = transform ? log1p(t * scale) : t;
    }
}

// the cell-order copy: entry k is entry perm[k] of the window order
__global__ void __launch_bounds__(LSI_BLOCK) lsi_transpose(const long long *__restrict__ perm, const int *__restrict__ erow,
                                                           const double *__restrict__ val, long long nnz, int *__restrict__ t_idx,
                                                           double *__restrict__ t_val) {
    for (long long k = (long long)blockIdx.x * LSI_BLOCK + threadIdx.x; k < nnz; k += (long long)gridDim.x * LSI_BLOCK) {
        const long long s = perm[k];
        t_idx[k] = erow[s];
        t_val[k] = val[s];
    }
}

// rows of q0 whose window is dropped are zero from the start
__global__ void __launch_bounds__(LSI_BLOCK) lsi_mask_rows(double *__restrict__ B, long long N, int r, const double *__restrict__ row_weight) {
    const long long total = N * r;
    for (long long t = (long long)blockIdx.x * LSI_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * LSI_BLOCK)
        if (!(row_weight[t / r] > 0.0)) B[t] = 0.0;
}

// *flag = 1 when B[0 .. total) holds anything but zeros (every writer stores the same word)
__global__ void __launch_bounds__(LSI_BLOCK) lsi_any_nonzero(const double *__restrict__ B, long long total, int *__restrict__ flag) {
    for (long long t = (long long)blockIdx.x * LSI_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * LSI_BLOCK)
        if (B[t] != 0.0) *flag = 1;
}

// the sum over the entries p, p + stride, ... < p1 of val * B[idx, j], in that order, four loads of B in flight
__device__ __forceinline__ double lsi_row_part(const int *__restrict__ idx, const double *__restrict__ val, long long p, long long p1,
                                               int stride, const double *__restrict__ B, int r, int j) {
    double acc = 0.0;
    const bool live = j < r;
    for (; p + 3LL * stride < p1; p += 4LL * stride) {
        const int i0 = idx[p], i1 = idx[p + stride], i2 = idx[p + 2LL * stride], i3 = idx[p + 3LL * stride];
        const double v0 = val[p], v1 = val[p + stride], v2 = val[p + 2LL * stride], v3 = val[p + 3LL * stride];
        const double b0 = live ? B[(size_t)i0 * r + j] : 0.0, b1 = live ? B[(size_t)i1 * r + j] : 0.0;
        const double b2 = live ? B[(size_t)i2 * r + j] : 0.0, b3 = live ? B[(size_t)i3 * r + j] : 0.0;
        acc = fma(v0, b0, acc);
        acc = fma(v1, b1, acc);
        acc = fma(v2, b2, acc);
        acc = fma(v3, b3, acc);
    }
    for (; p < p1; p += stride) {
        const double b = live ? B[(size_t)idx[p] * r + j] : 0.0;
        acc = fma(val[p], b, acc);
    }
    return acc;
}

// rows of at most LSI_SHORT_MAX entries (list[n_list], the empty ones among them): a lane group each
template <int RP>
__global__ void __launch_bounds__(LSI_BLOCK) lsi_spmm_short(const long long *__restrict__ list, long long n_list, const long long *__restrict__ ptr,
                                                            const int *__restrict__ idx, const double *__restrict__ val,
                                                            const double *__restrict__ B, int r, double *__restrict__ out) {
    constexpr int G = 64 / RP;
    const int lane = threadIdx.x & 63, j = lane & (RP - 1), g = lane / RP;
    const long long ngroups = (long long)gridDim.x * (LSI_BLOCK / 64) * G;
    for (long long k = ((long long)blockIdx.x * (LSI_BLOCK / 64) + (threadIdx.x >> 6)) * G + g; k < n_list; k += ngroups) {
        const long long i = list[k];
        const double acc = lsi_row_part(idx, val, ptr[i], ptr[i + 1], 1, B, r, j);
        if (j < r) out[(size_t)i * r + j] = acc;
    }
}

// the groups' sums of one wave, combined in every lane alike: (g, g ^ 1) pairs last
template <int RP>
__device__ __forceinline__ double lsi_combine_groups(double acc) {
#pragma unroll
    for (int off = 32; off >= RP; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// rows of LSI_SHORT_MAX + 1 .. LSI_WAVE_MAX entries: one wave each
template <int RP>
__global__ void __launch_bounds__(LSI_BLOCK) lsi_spmm_wave(const long long *__restrict__ list, long long n_list, const long long *__restrict__ ptr,
                                                           const int *__restrict__ idx, const double *__restrict__ val,
                                                           const double *__restrict__ B, int r, double *__restrict__ out) {
    constexpr int G = 64 / RP;
    const int lane = threadIdx.x & 63, j = lane & (RP - 1), g = lane / RP;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long nwaves = (long long)gridDim.x * (LSI_BLOCK / 64);
    for (long long k = (long long)blockIdx.x * (LSI_BLOCK / 64) + wave; k < n_list; k += nwaves) {      // wave-uniform: every lane shuffles
        const long long i = list[k];
        const double acc = lsi_combine_groups<RP>(lsi_row_part(idx, val, ptr[i] + g, ptr[i + 1], G, B, r, j));
        if (g == 0 && j < r) out[(size_t)i * r + j] = acc;
    }
}

// longer rows: one workgroup each
template <int RP>
__global__ void __launch_bounds__(LSI_BLOCK) lsi_spmm_block(const long long *__restrict__ list, long long n_list, const long long *__restrict__ ptr,
                                                            const int *__restrict__ idx, const double *__restrict__ val,
                                                            const double *__restrict__ B, int r, double *__restrict__ out) {
    constexpr int G = 64 / RP, NW = LSI_BLOCK / 64;
    __shared__ double s_part[NW][LSI_MAX_R];
    const int lane = threadIdx.x & 63, j = lane & (RP - 1), g = lane / RP;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long k = blockIdx.x; k < n_list; k += gridDim.x) {                                         // block-uniform
        const long long i = list[k];
        const double acc = lsi_combine_groups<RP>(lsi_row_part(idx, val, ptr[i] + wave * G + g, ptr[i + 1], NW * G, B, r, j));
        if (g == 0) s_part[wave][j] = acc;
        __syncthreads();
        if ((int)threadIdx.x < r) {
            const int t = threadIdx.x;
            out[(size_t)i * r + t] = ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
        }
        __syncthreads();                                    // the next row writes the same words
    }
}

// part[slab] (RP x RP, row-major) = the Gram matrix of the slab's rows of B (N x r), columns past r as zeros
template <int RP>
__global__ void __launch_bounds__(LSI_BLOCK) lsi_gram_slab(const double *__restrict__ B, long long N, int r, double *__restrict__ part) {
    constexpr int T = RP / 16;
    __shared__ double s[LSI_CHUNK][RP];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    const long long row0 = (long long)blockIdx.x * LSI_SLAB, row_end = row0 + LSI_SLAB < N ? row0 + LSI_SLAB : N;
    for (long long base = row0; base < row_end; base += LSI_CHUNK) {
        for (int q = threadIdx.x; q < LSI_CHUNK * RP; q += LSI_BLOCK) {
            const int rr = q / RP, cc = q & (RP - 1);
            const long long row = base + rr;
            s[rr][cc] = (row < row_end && cc < r) ? B[(size_t)row * r + cc] : 0.0;     // a zero row adds 0 * 0
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < LSI_CHUNK; ++k) {
            double av[T], bv[T];
#pragma unroll
            for (int a = 0; a < T; ++a) av[a] = s[k][ty * T + a];
#pragma unroll
            for (int b = 0; b < T; ++b) bv[b] = s[k][tx * T + b];
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
    double *o = part + (size_t)blockIdx.x * RP * RP;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) o[(ty * T + a) * RP + tx * T + b] = acc[a][b];
}

// G (r x r) = the partials added in slab order
__global__ void __launch_bounds__(LSI_BLOCK) lsi_gram_sum(const double *__restrict__ part, long long n_slab, int rp, int r, double *__restrict__ G) {
    const int t = blockIdx.x * LSI_BLOCK + threadIdx.x;
    if (t >= r * r) return;
    const int i = t / r, j = t - i * r;
    const double *p = part + (size_t)i * rp + j;
    double sum = 0.0;
#pragma unroll 8
    for (long long b = 0; b < n_slab; ++b) sum += p[(size_t)b * rp * rp];
    G[t] = sum;
}

// SOLVE: every row b of B (N x r) becomes the q with q R = b, R = M upper triangular (RP x RP, row-major, the identity past r):
//        q[j] = (b[j] - sum over k < j of q[k] R[k][j]) / R[j][j], k ascending.
// else:  every row b becomes b M (sum over k ascending), column j divided by d[j] where d is given.
template <int RP, bool SOLVE>
__global__ void __launch_bounds__(LSI_ROWS) lsi_rows_small(double *__restrict__ B, long long N, int r, const double *__restrict__ M,
                                                           const double *__restrict__ d) {
    constexpr int G = 64 / RP;
    __shared__ double s[LSI_ROWS][RP + 1];                 // + 1: a thread's row starts two banks after its neighbour's
    const int lane = threadIdx.x, j = lane & (RP - 1), g = lane / RP;
    const long long base = (long long)blockIdx.x * LSI_ROWS;
    for (int rr = g; rr < LSI_ROWS; rr += G) {
        const long long row = base + rr;
        s[rr][j] = (row < N && j < r) ? B[(size_t)row * r + j] : 0.0;
    }
    __syncthreads();
    double q[RP];
#pragma unroll
    for (int k = 0; k < RP; ++k) q[k] = s[lane][k];
#pragma unroll
    for (int jj = 0; jj < RP; ++jj) {
        if (jj < r) {                                       // uniform
            if (SOLVE) {
                double a = q[jj];
#pragma unroll
                for (int k = 0; k < jj; ++k) a = fma(-q[k], M[k * RP + jj], a);
                q[jj] = a / M[jj * RP + jj];
                s[lane][jj] = q[jj];
            } else {
                double a = 0.0;
#pragma unroll
                for (int k = 0; k < RP; ++k) a = fma(q[k], M[k * RP + jj], a);      // rows of M past r are zero, and so is q there
                s[lane][jj] = d ? a / d[jj] : a;
            }
        }
    }
    __syncthreads();
    for (int rr = g; rr < LSI_ROWS; rr += G) {
        const long long row = base + rr;
        if (row < N && j < r) B[(size_t)row * r + j] = s[rr][j];
    }
}

// ---- the host's r x r linear algebra ----
// Whether a Gram matrix G (r x r) is of a size the factorisation can work with: 0 yes; 2 no -- an entry is not finite, or the pivot floor
// r * eps * max(diag G) is below the smallest normal number; 3 its diagonal is zero: the block is empty or every square vanished.
static int lsi_gram_size(const std::vector<double> &G, int r) {
    for (const double g : G)
        if (!std::isfinite(g)) return 2;
    double dmax = 0.0;
    for (int i = 0; i < r; ++i) dmax = std::max(dmax, G[(size_t)i * r + i]);
    if (dmax == 0.0) return 3;
    return (double)r * std::numeric_limits<double>::epsilon() * dmax < std::numeric_limits<double>::min() ? 2 : 0;
}

// G (r x r, symmetric) = R^T R, R upper triangular, written into Rp (rp x rp, row-major, the identity past r).  false: a pivot is at most
// r * eps * max(diag G), or not a number -- the block has lost rank.
static bool lsi_cholesky(const std::vector<double> &G, int r, int rp, std::vector<double> &Rp) {
    Rp.assign((size_t)rp * rp, 0.0);
    for (int i = r; i < rp; ++i) Rp[(size_t)i * rp + i] = 1.0;
    double dmax = 0.0;
    for (int i = 0; i < r; ++i) {
        if (!std::isfinite(G[(size_t)i * r + i])) return false;
        dmax = std::max(dmax, G[(size_t)i * r + i]);
    }
    const double floor_ = (double)r * std::numeric_limits<double>::epsilon() * dmax;
    for (int j = 0; j < r; ++j) {
        double dd = G[(size_t)j * r + j];
        for (int k = 0; k < j; ++k) dd -= Rp[(size_t)k * rp + j] * Rp[(size_t)k * rp + j];
        if (!(dd > floor_)) return false;
        const double rjj = std::sqrt(dd);
        Rp[(size_t)j * rp + j] = rjj;
        for (int i = j + 1; i < r; ++i) {
            double v = G[(size_t)j * r + i];
            for (int k = 0; k < j; ++k) v -= Rp[(size_t)k * rp + j] * Rp[(size_t)k * rp + i];
            v /= rjj;
            if (!std::isfinite(v)) return false;
            Rp[(size_t)j * rp + i] = v;
        }
    }
    return true;
}

// cyclic Jacobi: A (r x r, symmetric; destroyed) = W diag(lam) W^T, lam descending (equal ones in their order on the diagonal), the
// columns of W (r x r, row-major) the eigenvectors
static void lsi_jacobi(std::vector<double> &A, int r, std::vector<double> &W, std::vector<double> &lam) {
    std::vector<double> Wt((size_t)r * r, 0.0);
    for (int i = 0; i < r; ++i) Wt[(size_t)i * r + i] = 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < r - 1; ++p)
            for (int q = p + 1; q < r; ++q) {
                const double apq = A[(size_t)p * r + q], app = A[(size_t)p * r + p], aqq = A[(size_t)q * r + q];
                // sqrt(|app|) * sqrt(|aqq|), not the root of the product: that is about sigma^4, out of range long before G is
                if (apq == 0.0 || std::fabs(apq) <= 0.125 * eps * (std::sqrt(std::fabs(app)) * std::sqrt(std::fabs(aqq)))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < r; ++k) {               // columns p and q
                    const double akp = A[(size_t)k * r + p], akq = A[(size_t)k * r + q];
                    A[(size_t)k * r + p] = cs * akp - sn * akq;
                    A[(size_t)k * r + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < r; ++k) {               // rows p and q
                    const double apk = A[(size_t)p * r + k], aqk = A[(size_t)q * r + k];
                    A[(size_t)p * r + k] = cs * apk - sn * aqk;
                    A[(size_t)q * r + k] = sn * apk + cs * aqk;
                }
                A[(size_t)p * r + q] = A[(size_t)q * r + p] = 0.0;
                for (int k = 0; k < r; ++k) {
                    const double wkp = Wt[(size_t)k * r + p], wkq = Wt[(size_t)k * r + q];
                    Wt[(size_t)k * r + p] = cs * wkp - sn * wkq;
                    Wt[(size_t)k * r + q] = sn * wkp + cs * wkq;
                }
            }
        if (!rotated) break;
    }
    std::vector<int> order((size_t)r);
    for (int i = 0; i < r; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * r + a] > A[(size_t)b * r + b]; });
    W.assign((size_t)r * r, 0.0);
    lam.assign((size_t)r, 0.0);
    for (int jn = 0; jn < r; ++jn) {
        const int jo = order[(size_t)jn];
        lam[(size_t)jn] = A[(size_t)jo * r + jo];
        for (int k = 0; k < r; ++k) W[(size_t)k * r + jn] = Wt[(size_t)k * r + jo];
    }
}

// one orientation of the matrix on the device: the rows' entries and the rows of every arm
struct LsiSide {
    const long long *ptr = nullptr;
    const int *idx = nullptr;
    const double *val = nullptr;
    const long long *list[3] = {nullptr, nullptr, nullptr};
    long long n_list[3] = {0, 0, 0};
};

// the rows of every arm by their length, in row order
static void lsi_row_arms(const long long *ptr, long long n_rows, std::vector<long long> arms[3]) {
    for (long long i = 0; i < n_rows; ++i) {
        const long long len = ptr[i + 1] - ptr[i];
        arms[len <= LSI_SHORT_MAX ? 0 : len <= LSI_WAVE_MAX ? 1 : 2].push_back(i);
    }
}

template <int RP>
static void lsi_spmm(hipStream_t st, const LsiSide &s, const double *B, int r, double *out) {
    constexpr int G = 64 / RP, NW = LSI_BLOCK / 64;
    if (s.n_list[0]) {
        const unsigned bx = (unsigned)std::min<long long>((s.n_list[0] + NW * G - 1) / (NW * G), 8192);
        hipLaunchKernelGGL((lsi_spmm_short<RP>), dim3(bx), dim3(LSI_BLOCK), 0, st, s.list[0], s.n_list[0], s.ptr, s.idx, s.val, B, r, out);
    }
    if (s.n_list[1]) {
        const unsigned bx = (unsigned)std::min<long long>((s.n_list[1] + NW - 1) / NW, 8192);
        hipLaunchKernelGGL((lsi_spmm_wave<RP>), dim3(bx), dim3(LSI_BLOCK), 0, st, s.list[1], s.n_list[1], s.ptr, s.idx, s.val, B, r, out);
    }
    if (s.n_list[2]) {
        const unsigned bx = (unsigned)std::min<long long>(s.n_list[2], 4096);
        hipLaunchKernelGGL((lsi_spmm_block<RP>), dim3(bx), dim3(LSI_BLOCK), 0, st, s.list[2], s.n_list[2], s.ptr, s.idx, s.val, B, r, out);
    }
}

template <int RP>
static void lsi_gram(hipStream_t st, const double *B, long long N, int r, double *part, double *G) {
    const long long n_slab = (N + LSI_SLAB - 1) / LSI_SLAB;
    hipLaunchKernelGGL((lsi_gram_slab<RP>), dim3((unsigned)n_slab), dim3(LSI_BLOCK), 0, st, B, N, r, part);
    hipLaunchKernelGGL(lsi_gram_sum, dim3((unsigned)((r * r + LSI_BLOCK - 1) / LSI_BLOCK)), dim3(LSI_BLOCK), 0, st, part, n_slab, RP, r, G);
}

template <int RP>
static void lsi_rows(hipStream_t st, bool solve, double *B, long long N, int r, const double *M, const double *d) {
    const unsigned bx = (unsigned)((N + LSI_ROWS - 1) / LSI_ROWS);
    if (solve) hipLaunchKernelGGL((lsi_rows_small<RP, true>), dim3(bx), dim3(LSI_ROWS), 0, st, B, N, r, M, d);
    else hipLaunchKernelGGL((lsi_rows_small<RP, false>), dim3(bx), dim3(LSI_ROWS), 0, st, B, N, r, M, d);
}

// the three padded widths behind one switch
#define NATAC_LSI_BY_WIDTH(rp, call)                                                                                                 \
    do {                                                                                                                             \
        if ((rp) == 16) { constexpr int RP = 16; call; }                                                                             \
        else if ((rp) == 32) { constexpr int RP = 32; call; }                                                                        \
        else { constexpr int RP = 64; call; }                                                                                        \
    } while (0)

}  // namespace natac_lsi

// ---- entry point -----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_sparse_lsi(natac_ctx *c, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                     const double *row_weight, const double *col_scale, double scale, int transform, int binarize, int r, int n_iter,
                     const double *q0, double *sigma, double *U, double *V, int32_t *status, double *kernel_ms) {
    using namespace natac_lsi;
    static_assert(LSI_MAX_R == NATAC_LSI_MAX_R && LSI_SHORT_MAX == NATAC_LSI_SHORT_MAX && LSI_WAVE_MAX == NATAC_LSI_WAVE_MAX,
                  "the arms' bounds are in natac.h");
    if (!c || !row_ptr || !sigma || !status) return fail(NATAC_E_ARG, "null argument");
    if (m < 0 || n < 0 || m > 2147483647LL || n > 2147483647LL) return fail(NATAC_E_ARG, "m and n must be in [0, 2^31)");
    if (r < 1 || r > LSI_MAX_R) return fail(NATAC_E_ARG, "r must be in [1, %d] (got %d)", LSI_MAX_R, r);
    if (n_iter < 1) return fail(NATAC_E_ARG, "n_iter must be at least 1 (got %d)", n_iter);
    if (transform != 0 && transform != 1) return fail(NATAC_E_ARG, "transform must be 0 (linear) or 1 (log) (got %d)", transform);
    if (!std::isfinite(scale) || scale < 0.0) return fail(NATAC_E_ARG, "scale must be finite and not negative");
    if ((m > 0 && (!row_weight || !q0 || !V)) || (n > 0 && (!col_scale || !U))) return fail(NATAC_E_ARG, "null argument");
    if (row_ptr[0] < 0) return fail(NATAC_E_ARG, "row_ptr[0] is negative");
    for (int64_t i = 0; i < m; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(NATAC_E_ARG, "row_ptr is not monotone (row %lld)", (long long)i);
    const int64_t e0 = row_ptr[0], nnz = row_ptr[m] - e0;
    if (nnz > 0 && (!col || !count)) return fail(NATAC_E_ARG, "null argument");
    for (int64_t i = 0; i < m; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(NATAC_E_ARG, "row %lld: column %d outside [0, %lld)", (long long)i, col[e], (long long)n);
            if (e > row_ptr[i] && col[e] <= col[e - 1]) return fail(NATAC_E_ARG, "row %lld: columns must be strictly ascending", (long long)i);
            if (count[e] < 1) return fail(NATAC_E_ARG, "row %lld: count %d is below 1", (long long)i, count[e]);
        }
    int64_t live_rows = 0, live_cols = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (!std::isfinite(row_weight[i]) || row_weight[i] < 0.0) return fail(NATAC_E_ARG, "row_weight[%lld] is negative or not finite", (long long)i);
        live_rows += row_weight[i] > 0.0;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(col_scale[i]) || col_scale[i] < 0.0) return fail(NATAC_E_ARG, "col_scale[%lld] is negative or not finite", (long long)i);
        live_cols += col_scale[i] > 0.0;
    }
    if (r > live_rows || r > live_cols)
        return fail(NATAC_E_ARG, "r (%d) is more than the %lld live rows or the %lld live columns", r, (long long)live_rows, (long long)live_cols);
    for (int64_t i = 0; i < m * r; ++i)
        if (!std::isfinite(q0[i])) return fail(NATAC_E_ARG, "q0[%lld] is not finite", (long long)i);
    if (kernel_ms) *kernel_ms = 0;
    *status = 0;
    // the cell-order copy's layout: a stable counting sort of the entries by cell (integers only; the header says why here)
    std::vector<long long> h_ptr((size_t)m + 1), t_ptr((size_t)n + 1, 0), perm((size_t)nnz);
    std::vector<int> erow((size_t)nnz);
    for (int64_t i = 0; i <= m; ++i) h_ptr[(size_t)i] = row_ptr[i] - e0;
    if (nnz) {
        col += e0;
        count += e0;
    }
    for (int64_t e = 0; e < nnz; ++e) ++t_ptr[(size_t)col[e] + 1];
    for (int64_t i = 0; i < n; ++i) t_ptr[(size_t)i + 1] += t_ptr[(size_t)i];
    {
        std::vector<long long> next(t_ptr.begin(), t_ptr.end() - 1);
        for (int64_t i = 0; i < m; ++i)
            for (long long e = h_ptr[(size_t)i]; e < h_ptr[(size_t)i + 1]; ++e) {
                perm[(size_t)next[(size_t)col[e]]++] = e;
                erow[(size_t)e] = (int)i;
            }
    }
    std::vector<long long> arms_a[3], arms_t[3];
    lsi_row_arms(h_ptr.data(), m, arms_a);
    lsi_row_arms(t_ptr.data(), n, arms_t);
    const int rp = r <= 16 ? 16 : r <= 32 ? 32 : 64;
    const long long n_slab_max = (std::max<long long>(m, n) + LSI_SLAB - 1) / LSI_SLAB;

    DeviceCall dc(c, "sparse_lsi");
    LsiSide A, T;                                           // A: rows are windows (X^T Y); T: rows are cells (X Q)
    A.ptr = dc.upload(h_ptr.data(), h_ptr.size());
    T.ptr = dc.upload(t_ptr.data(), t_ptr.size());
    A.idx = dc.upload((const int *)col, (size_t)nnz);
    const int *d_count = dc.upload((const int *)count, (size_t)nnz), *d_erow = dc.upload(erow.data(), (size_t)nnz);
    const long long *d_perm = dc.upload(perm.data(), (size_t)nnz);
    const double *d_rw = dc.upload(row_weight, (size_t)m), *d_cs = dc.upload(col_scale, (size_t)n);
    for (int a = 0; a < 3; ++a) {
        A.list[a] = dc.upload(arms_a[a].data(), arms_a[a].size());
        A.n_list[a] = (long long)arms_a[a].size();
        T.list[a] = dc.upload(arms_t[a].data(), arms_t[a].size());
        T.n_list[a] = (long long)arms_t[a].size();
    }
    double *d_val = dc.alloc<double>((size_t)nnz), *d_tval = dc.alloc<double>((size_t)nnz);
    int *d_tidx = dc.alloc<int>((size_t)nnz);
    A.val = d_val;
    T.idx = d_tidx;
    T.val = d_tval;
    double *d_Q = dc.upload(q0, (size_t)m * r), *d_Y = dc.alloc<double>((size_t)n * r);
    double *d_part = dc.alloc<double>((size_t)n_slab_max * rp * rp), *d_G = dc.alloc<double>((size_t)r * r);
    double *d_M = dc.alloc<double>((size_t)rp * rp), *d_M2 = dc.alloc<double>((size_t)rp * rp), *d_sig = dc.alloc<double>((size_t)rp);
    int *d_flag = dc.alloc<int>(1);
    hipStream_t st = c->stream;
    std::vector<double> hG((size_t)r * r), hR, hW, lam;

    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        if (nnz) {
            const unsigned bx = (unsigned)std::min<long long>((nnz + LSI_BLOCK - 1) / LSI_BLOCK, 16384);
            hipLaunchKernelGGL(lsi_weight, dim3(bx), dim3(LSI_BLOCK), 0, st, A.idx, d_count, d_erow, (long long)nnz, d_rw, d_cs, scale, transform,
                               binarize ? 1 : 0, d_val);
            hipLaunchKernelGGL(lsi_transpose, dim3(bx), dim3(LSI_BLOCK), 0, st, d_perm, d_erow, d_val, (long long)nnz, d_tidx, d_tval);
        }
        const unsigned bq = (unsigned)std::min<long long>((m * r + LSI_BLOCK - 1) / LSI_BLOCK, 16384);
        hipLaunchKernelGGL(lsi_mask_rows, dim3(bq), dim3(LSI_BLOCK), 0, st, d_Q, (long long)m, r, d_rw);
        dc.launched();
    }
    // a block whose Gram diagonal is zero: 1 it is zero itself (no direction), 2 it is not (its squares vanished), or an error code
    auto vanished = [&](const double *d_B, long long total) -> int {
        int h_flag = 0;
        dc.zero(d_flag, 1);
        if (dc.ok()) {
            const unsigned bx = (unsigned)std::min<long long>((total + LSI_BLOCK - 1) / LSI_BLOCK, 16384);
            hipLaunchKernelGGL(lsi_any_nonzero, dim3(bx), dim3(LSI_BLOCK), 0, st, d_B, total, d_flag);
            dc.launched();
        }
        dc.fetch(&h_flag, d_flag, 1);
        if (const int rc = dc.sync()) return rc;
        return h_flag ? 2 : 1;
    };
    // CholeskyQR2 of a block in place: 0, 1 (rank lost), 2 (out of range) or an error code.  hR is rewritten only behind a wait that has drained its last copy.
    auto orth = [&](double *d_B, long long N) -> int {
        for (int pass = 0; pass < 2; ++pass) {
            if (dc.ok()) {
                NATAC_LSI_BY_WIDTH(rp, lsi_gram<RP>(st, d_B, N, r, d_part, d_G));
                dc.launched();
            }
            dc.fetch(hG.data(), d_G, hG.size());
            if (const int rc = dc.sync()) return rc;
            if (const int size = lsi_gram_size(hG, r)) return size == 3 ? vanished(d_B, N * r) : size;
            if (!lsi_cholesky(hG, r, rp, hR)) return 1;
            dc.send(d_M, hR.data(), hR.size());
            if (dc.ok()) {
                NATAC_LSI_BY_WIDTH(rp, lsi_rows<RP>(st, true, d_B, N, r, d_M, nullptr));
                dc.launched();
            }
        }
        return 0;
    };
    auto product = [&](const LsiSide &s, const double *B, double *out) {
        if (!dc.ok()) return;
        NATAC_LSI_BY_WIDTH(rp, lsi_spmm<RP>(st, s, B, r, out));
        dc.launched();
    };
    auto lost = [&](int why) -> int {                      // the call is well, the basis is not
        dc.time_end();
        if (const int rc = dc.finish()) return rc;
        *status = why;
        for (int j = 0; j < r; ++j) sigma[j] = 0.0;
        for (int64_t i = 0; i < n * r; ++i) U[i] = 0.0;
        for (int64_t i = 0; i < m * r; ++i) V[i] = 0.0;
        return NATAC_OK;
    };
    int rc = orth(d_Q, m);
    for (int it = 0; it < n_iter && rc == 0; ++it) {
        product(T, d_Q, d_Y);
        if ((rc = orth(d_Y, n))) break;
        product(A, d_Y, d_Q);
        rc = orth(d_Q, m);
    }
    if (rc < 0) return rc;
    if (rc) return lost(rc);
    product(T, d_Q, d_Y);
    if (dc.ok()) {
        NATAC_LSI_BY_WIDTH(rp, lsi_gram<RP>(st, d_Y, n, r, d_part, d_G));
        dc.launched();
    }
    dc.fetch(hG.data(), d_G, hG.size());
    if ((rc = dc.sync())) return rc;
    if (int size = lsi_gram_size(hG, r)) {
        if (size == 3 && (size = vanished(d_Y, (long long)n * r)) < 0) return size;
        return lost(size);
    }
    lsi_jacobi(hG, r, hW, lam);
    for (int j = 0; j < r; ++j)
        if (!(lam[(size_t)j] > 0.0)) return lost(1);        // no direction left to divide by
    std::vector<double> hM((size_t)rp * rp, 0.0), hS((size_t)rp, 1.0);
    for (int k = 0; k < r; ++k)
        for (int j = 0; j < r; ++j) hM[(size_t)k * rp + j] = hW[(size_t)k * r + j];
    for (int j = 0; j < r; ++j) hS[(size_t)j] = sigma[j] = std::sqrt(lam[(size_t)j]);
    dc.send(d_M2, hM.data(), hM.size());
    dc.send(d_sig, hS.data(), hS.size());
    if (dc.ok()) {
        NATAC_LSI_BY_WIDTH(rp, lsi_rows<RP>(st, false, d_Y, n, r, d_M2, d_sig));
        NATAC_LSI_BY_WIDTH(rp, lsi_rows<RP>(st, false, d_Q, m, r, d_M2, nullptr));
        dc.launched();
    }
    dc.time_end();
    dc.fetch(U, d_Y, (size_t)n * r);
    dc.fetch(V, d_Q, (size_t)m * r);
    return dc.finish();
}

}  // extern "C"
