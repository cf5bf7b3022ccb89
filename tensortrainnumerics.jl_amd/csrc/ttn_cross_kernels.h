// ttn_cross_kernels.h — the device parts of TT-cross interpolation (src/tt_cross_interpolation.jl): the maxvol pivot search, the
// fibre / superblock index matrices with the coordinate gathers from the domain arrays, and the evaluation of a train at points
// (_evaluate_tt) or against one weight vector per site (_contract_with_weights).  Float64 or ComplexF64 (interleaved pairs),
// column-major matrices and 1-based int64 indices, as the reference holds them.  Self-contained: the header needs ttn_common.h only.
//
//   k_cross_maxvol   one m x r matrix A (m >= r) per launch, one workgroup.  Initial rows by LU with partial pivoting (getrf's choice:
//                    the first maximum of |Re| + |Im|), then swaps: (i, j) = argmax |C_ij| (complex modulus; ties to the smallest
//                    column-major index), stop when it is <= tol or after maxiter swaps, C = A / A[piv,:] kept by the Sherman-Morrison
//                    update of each swap (Goreinov et al. 2010; the algorithm of maxvolpy).  On exit C is computed again from scratch
//                    as A / A[piv,:] by an LU solve with the r x r block.  The working C lives in LDS when m r elements fit in 128 KiB,
//                    else in global memory: one code path over a pointer to either place.
//   k_cross_points   the P x N index matrix of a fibre (_build_fiber_indices order: i fastest, then r_left, then r_right), of a
//                    superblock (_sample_superblock order: r_l fastest, then i1, i2, r_g) or a given one, and the coordinates
//                    X[p, d] = domain_d[idx[p, d]] gathered from the concatenated domain arrays.
//   k_cross_eval     out[p] = prod_k core_k[idx[p, k], :, :] (point form) or prod_k (sum_i w_k[i] core_k[i, :, :]) with the running
//                    row conjugated before each factor, as `result' * contracted` does (weight form).  One wave per output.
//   k_cross_relerr   ||y - yhat|| / max(||y||, tol), one workgroup; entries scaled by a power of two before they are squared.
#pragma once
#include "ttn_common.h"
#include <climits>

#define TTN_XV_WG 1024                         // threads of k_cross_maxvol / k_cross_relerr
#define TTN_XV_MAX_R 1024                      // maxvol: r <= 1024, m <= 2^20
#define TTN_XV_MAX_M (1 << 20)
#define TTN_XV_LDS_C (128 * 1024)              // C in LDS when m r elements take at most this many bytes
#define TTN_XV_LDS_BYTES (TTN_XV_LDS_C + 16 * TTN_XV_MAX_R + 4 * TTN_XV_MAX_R)   // + the swap row + the column map of the final solve
#define TTN_XE_MAX_R 1024                      // evaluation: ranks up to 1024

template <bool CPLX> struct xvnum;
template <> struct xvnum<false> {
    typedef double T;
    static __device__ __forceinline__ T load(const double* p, long long i) { return p[i]; }
    static __device__ __forceinline__ void store(double* p, long long i, T v) { p[i] = v; }
    static __device__ __forceinline__ T zero() { return 0.0; }
    static __device__ __forceinline__ T one() { return 1.0; }
    static __device__ __forceinline__ T conj(T a) { return a; }
    static __device__ __forceinline__ T mul(T a, T b) { return a * b; }
    static __device__ __forceinline__ T fms(T c, T a, T b) { return fma(-a, b, c); }     // c - a b
    static __device__ __forceinline__ T fma_(T c, T a, T b) { return fma(a, b, c); }     // c + a b
    static __device__ __forceinline__ T sub(T a, T b) { return a - b; }
    static __device__ __forceinline__ T div(T a, T b) { return a / b; }
    static __device__ __forceinline__ T recip(T a) { return 1.0 / a; }
    static __device__ __forceinline__ double abs1(T a) { return fabs(a); }              // i?amax's measure
    static __device__ __forceinline__ double absv(T a) { return fabs(a); }
    static __device__ __forceinline__ double abs2(T a) { return a * a; }
    static __device__ __forceinline__ T ldexp_(T a, int e) { return ldexp(a, e); }
};
struct xvc { double x, y; };
template <> struct xvnum<true> {
    typedef xvc T;
    static __device__ __forceinline__ T load(const double* p, long long i) { return T{p[2 * i], p[2 * i + 1]}; }
    static __device__ __forceinline__ void store(double* p, long long i, T v) { p[2 * i] = v.x; p[2 * i + 1] = v.y; }
    static __device__ __forceinline__ T zero() { return T{0.0, 0.0}; }
    static __device__ __forceinline__ T one() { return T{1.0, 0.0}; }
    static __device__ __forceinline__ T conj(T a) { return T{a.x, -a.y}; }
    static __device__ __forceinline__ T mul(T a, T b) { return T{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }
    static __device__ __forceinline__ T fms(T c, T a, T b) { const T p = mul(a, b); return T{c.x - p.x, c.y - p.y}; }
    static __device__ __forceinline__ T fma_(T c, T a, T b) { const T p = mul(a, b); return T{c.x + p.x, c.y + p.y}; }
    static __device__ __forceinline__ T sub(T a, T b) { return T{a.x - b.x, a.y - b.y}; }
    static __device__ __forceinline__ T div(T a, T b) {                                  // Smith's algorithm
        if (fabs(b.x) >= fabs(b.y)) {
            const double t = b.y / b.x, d = b.x + b.y * t;
            return T{(a.x + a.y * t) / d, (a.y - a.x * t) / d};
        }
        const double t = b.x / b.y, d = b.y + b.x * t;
        return T{(a.x * t + a.y) / d, (a.y * t - a.x) / d};
    }
    static __device__ __forceinline__ T recip(T a) { return div(one(), a); }
    static __device__ __forceinline__ double abs1(T a) { return fabs(a.x) + fabs(a.y); }
    static __device__ __forceinline__ double absv(T a) { return hypot(a.x, a.y); }
    static __device__ __forceinline__ double abs2(T a) { return fma(a.x, a.x, a.y * a.y); }
    static __device__ __forceinline__ T ldexp_(T a, int e) { return T{ldexp(a.x, e), ldexp(a.y, e)}; }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// workgroup argmax: the larger value wins, equal values go to the smaller key; a NaN never wins.  rv / rk: LDS of >= 16 entries.
// Every thread returns the same pair.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool xv_better(double v, long long k, double bv, long long bk) { return v > bv || (v == bv && k < bk); }

__device__ inline void xv_argmax(double& v, long long& k, double* rv, long long* rk) {
    if (!(v >= 0.0)) { v = -1.0; k = LLONG_MAX; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const long long ok = __shfl_xor(k, off);
        if (xv_better(ov, ok, v, k)) { v = ov; k = ok; }
    }
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (l == 0) { rv[w] = v; rk[w] = k; }
    __syncthreads();
    v = -1.0; k = LLONG_MAX;
    for (int i = 0; i < nw; ++i)
        if (xv_better(rv[i], rk[i], v, k)) { v = rv[i]; k = rk[i]; }
    __syncthreads();                                   // rv / rk are free again
}

__device__ inline double xv_sum(double v, double* rv) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (l == 0) rv[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += rv[i];
    __syncthreads();
    return t;
}

// Unblocked LU with partial pivoting of W (m x r, leading dimension ld) in place, as getf2: per column the pivot is the FIRST
// maximum of |Re| + |Im| below the diagonal, the rows are swapped whole, the multipliers are the column times 1 / pivot.  perm
// (m entries, identity on entry) follows the swaps.  false: a zero (or NaN) pivot column; W and perm are then left mid-way.
template <bool CPLX>
__device__ bool xv_getf2(double* W, long long ld, int m, int r, int* perm, double* rv, long long* rk) {
    typedef xvnum<CPLX> N;
    typedef typename N::T T;
    const int tid = threadIdx.x, bs = blockDim.x;
    for (int j = 0; j < r; ++j) {
        double bv = -1.0;
        long long bk = LLONG_MAX;
        for (int i = j + tid; i < m; i += bs) {
            const double v = N::abs1(N::load(W, i + ld * j));
            if (xv_better(v, i, bv, bk)) { bv = v; bk = i; }
        }
        xv_argmax(bv, bk, rv, rk);
        if (!(bv > 0.0)) return false;
        const int p = (int)bk;
        if (p != j) {
            for (int c = tid; c < r; c += bs) {
                const T a = N::load(W, j + ld * c), b = N::load(W, p + ld * c);
                N::store(W, j + ld * c, b);
                N::store(W, p + ld * c, a);
            }
            if (tid == 0) { const int t = perm[j]; perm[j] = perm[p]; perm[p] = t; }
        }
        __syncthreads();
        const T inv = N::recip(N::load(W, j + ld * j));
        for (int i = j + 1 + tid; i < m; i += bs) N::store(W, i + ld * j, N::mul(N::load(W, i + ld * j), inv));
        __syncthreads();
        const long long rows = m - j - 1, cols = r - j - 1;
        for (long long t = tid; t < rows * cols; t += bs) {
            const long long i = j + 1 + t % rows, c = j + 1 + t / rows;
            N::store(W, i + ld * c, N::fms(N::load(W, i + ld * c), N::load(W, i + ld * j), N::load(W, j + ld * c)));
        }
        __syncthreads();
    }
    return true;
}

// C = A / A[piv,:] from scratch: B = A[piv,:] (r x r) is factorised in W (ld r) as P_b B = L U, then every row of A is solved,
// y (L U) = a, and C[:, sigma[k]] = y[k] (sigma: the rows of B in the order of P_b).  One thread per row.  false: B is singular.
template <bool CPLX>
__device__ bool xv_solve_final(int m, int r, const double* A, const long long* piv, double* C, double* W, int* perm, int* sigma,
                               double* rv, long long* rk) {
    typedef xvnum<CPLX> N;
    typedef typename N::T T;
    const int tid = threadIdx.x, bs = blockDim.x;
    for (long long t = tid; t < (long long)r * r; t += bs) {
        const long long i = t % r, c = t / r;
        N::store(W, i + (long long)r * c, N::load(A, (piv[i] - 1) + (long long)m * c));
    }
    for (int i = tid; i < r; i += bs) perm[i] = i;
    __syncthreads();
    if (!xv_getf2<CPLX>(W, r, r, r, perm, rv, rk)) return false;
    for (int i = tid; i < r; i += bs) sigma[i] = perm[i];
    __syncthreads();
    for (int i = tid; i < m; i += bs) {
        for (int k = 0; k < r; ++k) N::store(C, i + (long long)m * sigma[k], N::load(A, i + (long long)m * k));
        for (int q = 0; q < r; ++q) {                                  // z U = a
            T z = N::load(C, i + (long long)m * sigma[q]);
            for (int p = 0; p < q; ++p) z = N::fms(z, N::load(C, i + (long long)m * sigma[p]), N::load(W, p + (long long)r * q));
            N::store(C, i + (long long)m * sigma[q], N::div(z, N::load(W, q + (long long)r * q)));
        }
        for (int q = r - 1; q >= 0; --q) {                             // y L = z, L unit lower
            T y = N::load(C, i + (long long)m * sigma[q]);
            for (int p = q + 1; p < r; ++p) y = N::fms(y, N::load(C, i + (long long)m * sigma[p]), N::load(W, p + (long long)r * q));
            N::store(C, i + (long long)m * sigma[q], y);
        }
    }
    __syncthreads();
    return true;
}

// info[0]: 0 or TTN_ERR_SINGULAR's value (-10); info[1]: the number of swaps.  piv: r entries, 1-based, in column order; always
// rows of A (on a singular input: the rows chosen so far and the rest of the permutation), so that index gathers stay in range.
// Cw: m r numbers in global memory (used when use_lds = 0), perm: m ints of global memory.
template <bool CPLX>
__global__ void __launch_bounds__(TTN_XV_WG) k_cross_maxvol(int m, int r, const double* A, double tol, int maxiter, long long* piv, double* C,
                                                           double* Cw, int* perm, long long* info, int use_lds) {
    typedef xvnum<CPLX> N;
    typedef typename N::T T;
    extern __shared__ double xv_lds[];
    __shared__ double rv[TTN_XV_WG / 64];
    __shared__ long long rk[TTN_XV_WG / 64];
    const int tid = threadIdx.x, bs = blockDim.x;
    const long long ld = m;
    double* W = use_lds ? xv_lds : Cw;                                  // the working C: LDS or global, one code path
    double* rowk = xv_lds + (use_lds ? (CPLX ? 2 : 1) * (long long)m * r : 0);
    int* sigma = reinterpret_cast<int*>(rowk + (CPLX ? 2 : 1) * r);
    for (long long t = tid; t < (long long)m * r; t += bs) N::store(W, t, N::load(A, t));
    for (int i = tid; i < m; i += bs) perm[i] = i;
    __syncthreads();
    int swaps = 0;
    bool ok = xv_getf2<CPLX>(W, ld, m, r, perm, rv, rk);
    for (int j = tid; j < r; j += bs) piv[j] = perm[j] + 1;
    if (ok) {
        // C in the row order of the factorisation: rows r.. are L2 L1^-1 (solve x L1 = l in place), rows ..r the identity
        for (int i = r + tid; i < m; i += bs)
            for (int q = r - 1; q >= 0; --q) {
                T x = N::load(W, i + ld * q);
                for (int p = q + 1; p < r; ++p) x = N::fms(x, N::load(W, i + ld * p), N::load(W, p + ld * q));
                N::store(W, i + ld * q, x);
            }
        __syncthreads();
        for (long long t = tid; t < (long long)r * r; t += bs) {
            const long long i = t % r, c = t / r;
            N::store(W, i + ld * c, i == c ? N::one() : N::zero());
        }
        __syncthreads();
        // swaps: buffer row k holds row perm[k] of C; the search key is the column-major index in C's own row order
        while (swaps < maxiter) {
            double bv = -1.0;
            long long bk = LLONG_MAX;
            for (long long t = tid; t < (long long)m * r; t += bs) {
                const long long k = t % m, j = t / m;
                const double v = N::absv(N::load(W, t));
                const long long key = j * ld + perm[k];
                if (xv_better(v, key, bv, bk)) { bv = v; bk = key; }
            }
            // (the key names the row of C; the buffer row is found by the thread that holds it)
            xv_argmax(bv, bk, rv, rk);
            if (!(bv > tol)) break;
            const int j = (int)(bk / ld), row = (int)(bk % ld);
            __shared__ int kbuf;
            for (int k = tid; k < m; k += bs)
                if (perm[k] == row) kbuf = k;
            __syncthreads();
            const int k = kbuf;
            for (int c = tid; c < r; c += bs) N::store(rowk, c, N::load(W, k + ld * c));
            __syncthreads();
            const T inv = N::recip(N::load(rowk, j));
            for (int p = tid; p < m; p += bs) {                         // C -= C[:, j] (C[k, :] - e_j) / C[k, j]
                const T f = N::mul(N::load(W, p + ld * j), inv);
                for (int q = 0; q < r; ++q) {
                    T rq = N::load(rowk, q);
                    if (q == j) rq = N::sub(rq, N::one());
                    N::store(W, p + ld * q, N::fms(N::load(W, p + ld * q), f, rq));
                }
            }
            if (tid == 0) piv[j] = row + 1;
            ++swaps;
            __syncthreads();
        }
        // the returned C: A / A[piv, :] from scratch (the working copy is done with; its first r r numbers hold the LU of the block)
        ok = xv_solve_final<CPLX>(m, r, A, piv, C, W, perm, sigma, rv, rk);
    }
    if (!ok) {
        for (long long t = tid; t < (long long)m * r; t += bs) N::store(C, t, N::zero());
    }
    if (tid == 0) {
        info[0] = ok ? 0 : -10;
        info[1] = swaps;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// index matrices and coordinates.  mode 0: fibre of site `site` (1-based) with L (rl x (site-1)) and R (rr x (N-site));
// mode 1: superblock of sites site, site+1 with L (rl x (site-1)) and R (rr x (N-site-1)); mode 2: the given idx_in (P x N).
// doff: N + 1 offsets of the concatenated domain arrays; an index outside 1..n_d is clamped (never expected: the sets come from
// pivots).  idx_out / X may each be null.  One thread per entry (p, d).
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(256) k_cross_points(int mode, long long P, int N, int site, long long n1, long long n2, long long rl,
                                                      long long rr, const long long* L, const long long* R, const long long* idx_in,
                                                      const long long* doff, const double* dom, long long* idx_out, double* X) {
    typedef xvnum<CPLX> Nm;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P * N) return;
    const long long p = t % P;
    const int d = (int)(t / P);                      // 0-based axis
    const int s = site - 1;                          // 0-based site
    long long v;
    if (mode == 2) {
        v = idx_in[t];
    } else if (mode == 0) {
        const long long i = p % n1, q = p / n1, a = q % rl, b = q / rl;
        if (d < s) v = L[a + rl * d];
        else if (d == s) v = i + 1;
        else v = R[b + rr * (d - s - 1)];
    } else {
        const long long a = p % rl, q1 = p / rl, i1 = q1 % n1, q2 = q1 / n1, i2 = q2 % n2, g = q2 / n2;
        if (d < s) v = L[a + rl * d];
        else if (d == s) v = i1 + 1;
        else if (d == s + 1) v = i2 + 1;
        else v = R[g + rr * (d - s - 2)];
    }
    const long long len = doff[d + 1] - doff[d];
    v = v < 1 ? 1 : (v > len ? len : v);
    if (idx_out) idx_out[t] = v;
    if (X) Nm::store(X, t, Nm::load(dom, doff[d] + v - 1));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// train evaluation.  tab: [N] core pointers, [N] n_k, [N + 1] ranks, [N] offsets of the weight vectors in w.  weights == 0: the
// point form, row p of idx (P x N, 1-based) selects the slices; weights == 1: P = 1 and the slice of site k is sum_i w_k[i] core_k[i].
// One 64-lane workgroup per output; the running row (r <= 1024 numbers) in LDS, double-buffered.
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(64) k_cross_eval(int N, long long P, const long long* tab, const long long* idx, const double* w,
                                                  int weights, double* out) {
    typedef xvnum<CPLX> Nm;
    typedef typename Nm::T T;
    __shared__ double buf[2][(CPLX ? 2 : 1) * TTN_XE_MAX_R];
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= P) return;
    if (lane == 0) Nm::store(buf[0], 0, Nm::one());
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < N; ++k) {
        const double* core = reinterpret_cast<const double*>(tab[k]);
        const long long n = tab[N + k], ra = tab[2 * N + k], rb = tab[2 * N + k + 1];
        const double* wk = w ? w + (CPLX ? 2 : 1) * tab[3 * N + 1 + k] : nullptr;
        long long i0 = 0;
        if (!weights) {
            i0 = idx[p + P * k] - 1;
            i0 = i0 < 0 ? 0 : (i0 >= n ? n - 1 : i0);
        }
        for (long long b = lane; b < rb; b += 64) {
            T acc = Nm::zero();
            for (long long a = 0; a < ra; ++a) {
                T s = Nm::load(buf[cur], a);
                T m;
                if (!weights) {
                    m = Nm::load(core, i0 + n * (a + ra * b));
                } else {
                    s = Nm::conj(s);
                    m = Nm::zero();
                    for (long long i = 0; i < n; ++i) m = Nm::fma_(m, Nm::load(wk, i), Nm::load(core, i + n * (a + ra * b)));
                }
                acc = Nm::fma_(acc, s, m);
            }
            Nm::store(buf[cur ^ 1], b, acc);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (lane == 0) Nm::store(out, p, Nm::load(buf[cur], 0));
}

// err[0] = ||y - yhat|| / max(||y||, tol).  Every entry is scaled by 2^-e before it is squared, 2^e the binade of the largest modulus
// of y and y - yhat (ldexp: exact, no overflow or underflow of the squares), and the ratio is taken in the scaled units:
// ||d|| / max(||y||, tol) = ||2^-e d|| / max(||2^-e y||, 2^-e tol).
template <bool CPLX>
__global__ void __launch_bounds__(TTN_XV_WG) k_cross_relerr(long long P, const double* y, const double* yhat, double tol, double* err) {
    typedef xvnum<CPLX> Nm;
    typedef typename Nm::T T;
    __shared__ double rv[TTN_XV_WG / 64];
    __shared__ long long rk[TTN_XV_WG / 64];
    double big = 0.0;
    long long key = 0;
    for (long long p = threadIdx.x; p < P; p += blockDim.x) {
        const T a = Nm::load(y, p);
        big = fmax(big, fmax(Nm::absv(a), Nm::absv(Nm::sub(a, Nm::load(yhat, p)))));
    }
    xv_argmax(big, key, rv, rk);
    const int e = (big > 0.0 && big <= 1.7976931348623157e308) ? ilogb(big) : 0;
    double num = 0.0, den = 0.0;
    for (long long p = threadIdx.x; p < P; p += blockDim.x) {
        const T a = Nm::load(y, p);
        num += Nm::abs2(Nm::ldexp_(Nm::sub(a, Nm::load(yhat, p)), -e));
        den += Nm::abs2(Nm::ldexp_(a, -e));
    }
    num = xv_sum(num, rv);
    den = xv_sum(den, rv);
    if (threadIdx.x == 0) err[0] = sqrt(num) / fmax(sqrt(den), ldexp(tol, -e));
}
