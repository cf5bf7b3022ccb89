// ttn_cross_batch_kernels.h — MaxVol cross for a batch of functions (tt_cross_batch): the kernels of ttn_cross_kernels.h with a leading
// function axis, and one kernel that does a whole site step.  Float64 only.  Per-function arrays are contiguous, function a at a times
// the size of one; matrices column-major, indices int64 and 1-based.
//
//   k_cross_batch_points  the index matrix and coordinates of the fibre of one site for every function from its own left and right
//                         sets (mode 0, the order of k_cross_points), or the coordinates of one shared index matrix written once per
//                         function (mode 2).  Grid (entries, functions).
//   k_cross_batch_site    one 1024-thread workgroup per function: the m x r fibre matrix read from the values as f returned them
//                         (left-to-right the plain reshape, right-to-left the transpose of the permuted tensor, by indexing), scaled
//                         by the power of two of its largest modulus, Householder QR in the operation order of k_dense_qr, the pivot
//                         search of k_cross_maxvol (same device functions), the core in the layout k_cross_eval reads, the next
//                         index set written to the per-function set array, {status, swaps}.  The fibre matrix (afterwards the working
//                         C) and Q live in LDS when 2 * 8 * m * r bytes fit TTN_XB_LDS_MAT, else in a per-function slice of
//                         workspace: one code path over a pointer.
//   k_cross_batch_eval    k_cross_eval for A trains whose cores are [A][n r_left r_right] per site, at one shared index matrix or
//                         against the weights: one wave per (point, function).
//   k_cross_batch_relerr  k_cross_relerr per function.
#pragma once
#include "ttn_cross_kernels.h"

#define TTN_XB_WG 1024
#define TTN_XB_LDS_MAT (144 * 1024)                     // the two m x r matrices in LDS when they take at most this many bytes
#define TTN_XB_LDS_SMALL(r) (20 * (size_t)(r))          // taus, the swap row (doubles) and the column map (ints)
#define TTN_XB_LDS_BYTES (TTN_XB_LDS_MAT + 4096)        // (in LDS r <= 96; with the matrices in workspace 20 r <= 20 KiB)
#define TTN_XB_MAX_A 65535                              // functions per launch (a grid dimension)

__global__ void __launch_bounds__(256) k_cross_batch_points(int mode, long long P, int N, int site, long long n1, long long rl, long long rr,
                                                            const long long* L, const long long* R, const long long* idx_in,
                                                            const long long* doff, const double* dom, long long* idx_out, double* X) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P * N) return;
    const long long a = blockIdx.y;
    const long long p = t % P;
    const int d = (int)(t / P);                      // 0-based axis
    const int s = site - 1;                          // 0-based site
    long long v;
    if (mode == 2) {
        v = idx_in[t];
    } else {
        const long long i = p % n1, q = p / n1, il = q % rl, ir = q / rl;
        if (d < s) v = L[a * rl * s + il + rl * d];
        else if (d == s) v = i + 1;
        else v = R[a * rr * (N - site) + ir + rr * (d - s - 1)];
    }
    const long long len = doff[d + 1] - doff[d];
    v = v < 1 ? 1 : (v > len ? len : v);
    if (idx_out) idx_out[a * P * N + t] = v;
    if (X) X[a * P * N + t] = dom[doff[d] + v - 1];
}

// Householder QR of Am (m x r, m >= r, column-major, overwritten by the reflectors) into Q (m x r): geqr2 + org2r with the
// statements of k_dense_qr<false> (the column norms are reduced by xv_sum).  taus: r doubles; red: >= 16 doubles, sh: 8 doubles of LDS.
__device__ inline void xb_qr(int m, int r, double* Am, double* Q, double* taus, double* red, double* sh) {
    const int tid = threadIdx.x;
    for (int k = 0; k < r; ++k) {
        double part = 0.0;
        for (int i = k + 1 + tid; i < m; i += TTN_XB_WG) { const double x = Am[i + (long long)m * k]; part += x * x; }
        const double xnorm2 = xv_sum(part, red);
        const double alpha = Am[k + (long long)m * k];
        if (tid == 0) {
            double tau = 0.0, beta = alpha, scal = 0.0;
            if (xnorm2 != 0.0) {
                beta = -copysign(sqrt(alpha * alpha + xnorm2), alpha);
                tau = (beta - alpha) / beta;
                const double den = alpha - beta, d2 = den * den;
                scal = den / d2;
            }
            taus[k] = tau;
            sh[0] = scal; sh[2] = beta; sh[3] = tau;
        }
        __syncthreads();
        const double scal = sh[0], tau = sh[3], beta = sh[2];
        const bool trivial = (tau == 0.0);
        if (!trivial)
            for (int i = k + 1 + tid; i < m; i += TTN_XB_WG) Am[i + (long long)m * k] = Am[i + (long long)m * k] * scal;
        __syncthreads();
        if (!trivial) {
            for (int j = k + 1 + tid; j < r; j += TTN_XB_WG) {
                double w = Am[k + (long long)m * j];
                for (int i = k + 1; i < m; ++i) w = w + Am[i + (long long)m * k] * Am[i + (long long)m * j];
                const double tw = tau * w;
                Am[k + (long long)m * j] = Am[k + (long long)m * j] - tw;
                for (int i = k + 1; i < m; ++i) Am[i + (long long)m * j] = Am[i + (long long)m * j] - tw * Am[i + (long long)m * k];
            }
        }
        if (tid == 0) Am[k + (long long)m * k] = beta;
        __syncthreads();
    }
    for (long long e = tid; e < (long long)m * r; e += TTN_XB_WG) Q[e] = (e % m == e / m) ? 1.0 : 0.0;
    __syncthreads();
    for (int k = r - 1; k >= 0; --k) {
        const double tau = taus[k];
        if (tau != 0.0) {
            for (int j = k + tid; j < r; j += TTN_XB_WG) {
                double w = Q[k + (long long)m * j];
                for (int i = k + 1; i < m; ++i) w = w + Am[i + (long long)m * k] * Q[i + (long long)m * j];
                const double tw = tau * w;
                Q[k + (long long)m * j] = Q[k + (long long)m * j] - tw;
                for (int i = k + 1; i < m; ++i) Q[i + (long long)m * j] = Q[i + (long long)m * j] - tw * Am[i + (long long)m * k];
            }
        }
        __syncthreads();
    }
}

// maxvol of Q (m x r) with the rules of k_cross_maxvol<false>: W (m r doubles) is the working C, piv receives the r rows (1-based),
// C = Q / Q[piv,:] solved from scratch.  Returns false on a zero pivot (C is then left to the caller); swaps: the number of swaps.
__device__ inline bool xb_maxvol(int m, int r, const double* Q, double* W, double tol, int maxiter, long long* piv, double* C, int* perm,
                                 double* rowk, int* sigma, double* rv, long long* rk, int* kbuf, int& swaps) {
    const int tid = threadIdx.x, bs = blockDim.x;
    const long long ld = m;
    for (long long t = tid; t < (long long)m * r; t += bs) W[t] = Q[t];
    for (int i = tid; i < m; i += bs) perm[i] = i;
    __syncthreads();
    swaps = 0;
    bool ok = xv_getf2<false>(W, ld, m, r, perm, rv, rk);
    for (int j = tid; j < r; j += bs) piv[j] = perm[j] + 1;
    if (!ok) return false;
    for (int i = r + tid; i < m; i += bs)
        for (int q = r - 1; q >= 0; --q) {
            double x = W[i + ld * q];
            for (int p = q + 1; p < r; ++p) x = fma(-W[i + ld * p], W[p + ld * q], x);
            W[i + ld * q] = x;
        }
    __syncthreads();
    for (long long t = tid; t < (long long)r * r; t += bs) W[t % r + ld * (t / r)] = (t % r == t / r) ? 1.0 : 0.0;
    __syncthreads();
    while (swaps < maxiter) {
        double bv = -1.0;
        long long bk = LLONG_MAX;
        for (long long t = tid; t < (long long)m * r; t += bs) {
            const long long k = t % m, j = t / m;
            const double v = fabs(W[t]);
            const long long key = j * ld + perm[k];
            if (xv_better(v, key, bv, bk)) { bv = v; bk = key; }
        }
        xv_argmax(bv, bk, rv, rk);
        if (!(bv > tol)) break;
        const int j = (int)(bk / ld), row = (int)(bk % ld);
        for (int k = tid; k < m; k += bs)
            if (perm[k] == row) *kbuf = k;
        __syncthreads();
        const int k = *kbuf;
        for (int c = tid; c < r; c += bs) rowk[c] = W[k + ld * c];
        __syncthreads();
        const double inv = 1.0 / rowk[j];
        for (int p = tid; p < m; p += bs) {                             // C -= C[:, j] (C[k, :] - e_j) / C[k, j]
            const double f = W[p + ld * j] * inv;
            for (int q = 0; q < r; ++q) {
                double rq = rowk[q];
                if (q == j) rq = rq - 1.0;
                W[p + ld * q] = fma(-f, rq, W[p + ld * q]);
            }
        }
        if (tid == 0) piv[j] = row + 1;
        ++swaps;
        __syncthreads();
    }
    return xv_solve_final<false>(m, r, Q, piv, C, W, perm, sigma, rv, rk);
}

// One site step per function.  dir 0 (left-to-right): m = rl n rows, r = rr columns, set_in = lsets[site] (rl x nin, nin = site - 1),
// set_out = lsets[site + 1] (r x (nin + 1)); dir 1 (right-to-left): m = n rr rows, r = rl columns, set_in = rsets[site] (rr x nin,
// nin = N - site), set_out = rsets[site - 1] (r x (nin + 1)).  V: [A][rl n rr] in fibre order (i fastest, then the left, then the right
// rank index); core: [A][n rl rr] as (n, rl, r) or (n, r, rr); piv: [A][r]; info: [A][2].  ws: ws_stride doubles per function:
// the two matrices when use_lds = 0, then m r doubles of the unpermuted C when dir = 1, then m ints.
__global__ void __launch_bounds__(TTN_XB_WG) k_cross_batch_site(int dir, int n, int rl, int rr, int nin, const double* V, double tol, int maxiter,
                                                               const long long* set_in, long long* set_out, double* core, long long* piv,
                                                               long long* info, double* ws, long long ws_stride, int use_lds) {
    extern __shared__ double xb_lds[];
    __shared__ double rv[TTN_XB_WG / 64];
    __shared__ long long rk[TTN_XB_WG / 64];
    __shared__ double sh[8];
    __shared__ int kbuf;
    const int tid = threadIdx.x, bs = blockDim.x;
    const long long a = blockIdx.x;
    const int m = dir == 0 ? rl * n : n * rr, r = dir == 0 ? rr : rl;
    const long long sz = (long long)m * r;
    double* wsf = ws + a * ws_stride;
    double* Am = use_lds ? xb_lds : wsf;
    double* Q = Am + sz;
    double* small_ = use_lds ? xb_lds + 2 * sz : xb_lds;
    double* taus = small_;
    double* rowk = small_ + r;
    int* sigma = reinterpret_cast<int*>(small_ + 2 * (long long)r);
    double* Ct = wsf + (use_lds ? 0 : 2 * sz);
    int* perm = reinterpret_cast<int*>(Ct + (dir == 0 ? 0 : sz));
    const double* Vf = V + a * sz;
    double* coref = core + a * sz;
    long long* pivf = piv + a * r;

    // ---- the fibre matrix, scaled by 2^-e, 2^e the binade of its largest modulus ----
    double big = 0.0;
    for (long long t = tid; t < sz; t += bs) big = fmax(big, fabs(Vf[t]));
    long long key = 0;
    xv_argmax(big, key, rv, rk);
    int e = 0;
    if (big > 0.0) {
        e = ilogb(big);
        e = e < -1022 ? -1022 : (e > 1023 ? 1023 : e);
    }
    // An all-zero fibre has no pivots to offer (its Q would be columns of the identity, whatever the function is elsewhere): it is
    // reported as singular, with the rows 1..r as in-range pivots.
    int swaps = 0;
    bool ok = big > 0.0;
    if (ok) {
        for (long long t = tid; t < sz; t += bs) {
            const long long row = t % m, col = t / m;
            long long src = t;
            if (dir != 0) { const long long i = row % n, b = row / n; src = i + n * (col + (long long)rl * b); }
            Am[t] = ldexp(Vf[src], -e);
        }
        __syncthreads();
        xb_qr(m, r, Am, Q, taus, rv, sh);
        ok = xb_maxvol(m, r, Q, Am, tol, maxiter, pivf, dir == 0 ? coref : Ct, perm, rowk, sigma, rv, rk, &kbuf, swaps);
    } else {
        for (int j = tid; j < r; j += bs) pivf[j] = j + 1;
    }
    if (!ok) {
        for (long long t = tid; t < sz; t += bs) coref[t] = 0.0;
    } else if (dir != 0) {
        for (long long t = tid; t < sz; t += bs) {                      // core (n, r, rr): [i, c, b] = C[i + n b, c]
            const long long i = t % n, q = t / n, c = q % r, b = q / r;
            coref[t] = Ct[(i + n * b) + (long long)m * c];
        }
    }
    __syncthreads();                                                    // the pivots are visible to the workgroup

    // ---- the next index set ----
    const long long rin = dir == 0 ? rl : rr;
    const long long* sin = set_in ? set_in + a * rin * nin : nullptr;
    long long* sout = set_out + a * (long long)r * (nin + 1);
    for (long long t = tid; t < (long long)r * (nin + 1); t += bs) {
        const long long c = t % r, d = t / r, p = pivf[c] - 1;
        const long long li = p % n + 1, lr = p / n;
        long long v;
        if (dir == 0) v = d < nin ? sin[lr + rin * d] : li;
        else v = d == 0 ? li : sin[lr + rin * (d - 1)];
        sout[t] = v;
    }
    if (tid == 0) {
        info[2 * a] = ok ? 0 : -10;
        info[2 * a + 1] = swaps;
    }
}

// tab: [N] addresses of the per-site core arrays ([A][n_k r_{k-1} r_k]), [N] n_k, [N + 1] ranks, [N] offsets of the weight vectors.
// Grid (P, A), one wave each; out: [A][P].
__global__ void __launch_bounds__(64) k_cross_batch_eval(int N, long long P, const long long* tab, const long long* idx, const double* w,
                                                        int weights, double* out) {
    __shared__ double buf[2][TTN_XE_MAX_R];
    const long long p = blockIdx.x, f = blockIdx.y;
    const int lane = threadIdx.x;
    if (lane == 0) buf[0][0] = 1.0;
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < N; ++k) {
        const long long n = tab[N + k], ra = tab[2 * N + k], rb = tab[2 * N + k + 1];
        const double* core = reinterpret_cast<const double*>(tab[k]) + f * n * ra * rb;
        const double* wk = w ? w + tab[3 * N + 1 + k] : nullptr;
        long long i0 = 0;
        if (!weights) {
            i0 = idx[p + P * k] - 1;
            i0 = i0 < 0 ? 0 : (i0 >= n ? n - 1 : i0);
        }
        for (long long b = lane; b < rb; b += 64) {
            double acc = 0.0;
            for (long long a = 0; a < ra; ++a) {
                double mm;
                if (!weights) {
                    mm = core[i0 + n * (a + ra * b)];
                } else {
                    mm = 0.0;
                    for (long long i = 0; i < n; ++i) mm = fma(wk[i], core[i + n * (a + ra * b)], mm);
                }
                acc = fma(buf[cur][a], mm, acc);
            }
            buf[cur ^ 1][b] = acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (lane == 0) out[f * P + p] = buf[cur][0];
}

// err[a] = ||y_a - yhat_a|| / max(||y_a||, tol) with the power-of-two scaling of k_cross_relerr; y, yhat: [A][P].  One workgroup each.
__global__ void __launch_bounds__(TTN_XB_WG) k_cross_batch_relerr(long long P, const double* y, const double* yhat, double tol, double* err) {
    __shared__ double rv[TTN_XB_WG / 64];
    __shared__ long long rk[TTN_XB_WG / 64];
    const double* ya = y + (long long)blockIdx.x * P;
    const double* ha = yhat + (long long)blockIdx.x * P;
    double big = 0.0;
    long long key = 0;
    for (long long p = threadIdx.x; p < P; p += blockDim.x) big = fmax(big, fmax(fabs(ya[p]), fabs(ya[p] - ha[p])));
    xv_argmax(big, key, rv, rk);
    const int e = (big > 0.0 && big <= 1.7976931348623157e308) ? ilogb(big) : 0;
    double num = 0.0, den = 0.0;
    for (long long p = threadIdx.x; p < P; p += blockDim.x) {
        const double dd = ldexp(ya[p] - ha[p], -e), yy = ldexp(ya[p], -e);
        num += dd * dd;
        den += yy * yy;
    }
    num = xv_sum(num, rv);
    den = xv_sum(den, rv);
    if (threadIdx.x == 0) err[blockIdx.x] = sqrt(num) / fmax(sqrt(den), ldexp(tol, -e));
}
