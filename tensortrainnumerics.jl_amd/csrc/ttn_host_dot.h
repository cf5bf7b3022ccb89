// ttn_host_dot.h — host API: dot, norm, <x, A y>, orthogonalize and the timing / state queries of their launches.
#ifndef TTN_HOST_DOT_H
#define TTN_HOST_DOT_H
#include "ttn_host_core.h"
#include "ttn_dot_kernels.h"
#include "ttn_cplx_kernels.h"
#include "ttn_expect_kernels.h"
#include "ttn_ortho_kernels.h"
#include "ttn_ortho512.h"
#include "ttn_ortho_ramp.h"

namespace {
size_t g_ortho_state_off = 0;     // byte offset in g_scratch of the state words of the last ttn_orthogonalize (ttn_debug_ortho_state)
int g_ortho_state_batch = 0;      // its batch; 0: none
}  // namespace

extern "C" {
// dot on ComplexF64 handles (k_zdot): out receives `batch` interleaved (re, im) pairs
static int zdot(ttn_tt_t a, ttn_tt_t b, double* out) {
    const int d = a->d;
    long long wmax = 1, tmax = 1;
    for (int m = 0; m <= d; ++m) wmax = std::max<long long>(wmax, a->bound[m] * b->bound[m]);
    for (int k = 0; k < d; ++k) tmax = std::max<long long>(tmax, a->dims[k] * a->bound[k] * b->bound[k + 1]);
    const long long per_train = 2 * (wmax + tmax);
    const int in_lds = per_train <= TTN_ZDOT_LDS_DOUBLES ? 1 : 0;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * a->batch);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * 2 * a->batch);
    if (rc) return rc;
    ZDotArgs P;
    P.a = a->dev(); P.b = b->dev();
    P.scratch = g_scratch.as<double>(); P.scratch_stride = per_train;
    P.wmax = wmax; P.tmax = tmax; P.in_lds = in_lds;
    P.out = g_dout.as<double>();
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    hipLaunchKernelGGL(k_zdot, dim3(a->batch), dim3(TTN_ZC_WG), in_lds ? sizeof(double) * (size_t)per_train : 0, g_stream, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * 2 * a->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

int ttn_dot(ttn_tt_t a, ttn_tt_t b, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!a || !b || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (!same_dims(a->dims, b->dims)) return fail(TTN_ERR_DIMS, "TT dimensions are not compatible");
    if (a->batch != b->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (a->el != b->el) return refuse_mixed("ttn_dot");
    if (a->el == 2) return zdot(a, b, out);
    const int d = a->d;
    if (d > DOT_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_dot: chains longer than 480 sites are not supported");
    if (a->stride >= (1LL << 31) || b->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_dot: a train of 2^31 doubles or more");
    long long ramax = 1, rbmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) { ramax = std::max<long long>(ramax, a->bound[m]); rbmax = std::max<long long>(rbmax, b->bound[m]); }
    for (int k = 0; k < d; ++k) nmax = std::max<long long>(nmax, a->dims[k]);
    const long long per_train = (2 + nmax) * ramax * rbmax + 16;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * a->batch);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * a->batch);
    if (rc) return rc;
    DotArgs P;
    P.a = a->dev(); P.b = b->dev();
    P.scratch = g_scratch.as<double>(); P.scratch_stride = per_train;
    P.ramax = (int)ramax; P.rbmax = (int)rbmax; P.nmax = (int)nmax;
    P.out = g_dout.as<double>();
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    hipLaunchKernelGGL(k_dot_fused, dim3(a->batch), dim3(TTN_WG), DOT_LDS_BYTES(d), g_stream, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));       // ttn_last_launch_ms: the kernel alone (this call goes on to copy and synchronise)
    g_have_launch_ms = true;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * a->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// <x, A y> (include/ttn_expect.h): k_expect, one workgroup per train; d_out is device memory
static_assert(EXPECT_QTT_RMAX == TTN_EXPECT_QTT_MAX_RANK && EXPECT_QTT_OPR_MAX == TTN_EXPECT_QTT_MAX_OP_RANK, "ttn_expect.h and ttn_expect_kernels.h disagree");
static int sandwich_launch(const char* who, ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out) {
    F64_ONLY(who, {x, y}, {A});
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (int rb = op_batch_fits(A, x->batch)) return rb;
    const int d = x->d;
    if (d > EXPECT_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich: chains longer than 480 sites are not supported");
    if (x->stride >= (1LL << 31) || y->stride >= (1LL << 31) || A->off.back() >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich: a train or an operator of 2^31 doubles or more");
    long long rxmax = 1, rymax = 1, Rmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) {
        rxmax = std::max<long long>(rxmax, x->bound[m]); rymax = std::max<long long>(rymax, y->bound[m]); Rmax = std::max<long long>(Rmax, A->rks[m]);
    }
    bool qtt = Rmax <= EXPECT_QTT_OPR_MAX;
    for (int k = 0; k < d; ++k) { nmax = std::max<long long>(nmax, x->dims[k]); qtt = qtt && x->dims[k] == 2; }
    // 32-bit element offsets in the workgroup GEMM: the workspace of one train stays below 2^31 doubles
    if (rxmax >= (1LL << 31) || rymax >= (1LL << 31) || Rmax >= (1LL << 31) || rxmax * rymax >= (1LL << 31) || rxmax * rymax * Rmax >= (1LL << 31)
        || (2 + 2 * nmax) * rxmax * rymax * Rmax >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich: ranks too large (the three-layer state of one train reaches 2^31 doubles)");
    const long long general = (2 + 2 * nmax) * rxmax * rymax * Rmax;
    const long long per_train = std::max<long long>(general, qtt ? Rmax * EXPECT_IMG_STATE : 0) + 16;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * x->batch);
    if (rc) return rc;
    ExpectArgs P;
    P.x = x->dev(); P.y = y->dev(); P.A = A->dev();
    P.scratch = g_scratch.as<double>(); P.scratch_stride = per_train;
    P.rxmax = (int)rxmax; P.rymax = (int)rymax; P.Rmax = (int)Rmax; P.nmax = (int)nmax;
    P.out = d_out;
    const dim3 grid(x->batch), block(TTN_WG);
    const size_t lds = EXPECT_LDS_BYTES(d);
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    switch (qtt ? (int)Rmax : 0) {
        case 1: hipLaunchKernelGGL(k_expect<1>, grid, block, lds, g_stream, P); break;
        case 2: hipLaunchKernelGGL(k_expect<2>, grid, block, lds, g_stream, P); break;
        case 3: hipLaunchKernelGGL(k_expect<3>, grid, block, lds, g_stream, P); break;
        case 4: hipLaunchKernelGGL(k_expect<4>, grid, block, lds, g_stream, P); break;
        case 5: hipLaunchKernelGGL(k_expect<5>, grid, block, lds, g_stream, P); break;
        default: hipLaunchKernelGGL(k_expect<0>, grid, block, lds, g_stream, P); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    return TTN_OK;
}

int ttn_sandwich_dev(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !A || !y || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    return sandwich_launch("ttn_sandwich_dev", x, A, y, d_out);
}

int ttn_sandwich(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !A || !y || !out) return fail(TTN_ERR_ARG, "null pointer");
    int rc = g_dout.ensure(sizeof(double) * x->batch);
    if (rc) return rc;
    if ((rc = sandwich_launch("ttn_sandwich", x, A, y, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * x->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// diagnostics: the per-train state words of the last orthogonalize (next site, buffers, sites taken by k_ortho512), read from the
// workspace where that call left them (the workspace only grows, so the words stay in bounds until ttn_finalize)
int ttn_debug_ortho_state(int64_t b, int64_t* out4) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!out4 || b < 0 || b >= g_ortho_state_batch) return fail(TTN_ERR_ARG, "ttn_debug_ortho_state: no orthogonalize of a batch with train b yet");
    int tmp[4];
    HIPCHK(hipMemcpyAsync(tmp, g_scratch.as<char>() + g_ortho_state_off + sizeof(tmp) * b, sizeof(tmp), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int i = 0; i < 4; ++i) out4[i] = tmp[i];
    return TTN_OK;
}

int ttn_last_launch_ms(float* ms) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!ms) return fail(TTN_ERR_ARG, "null pointer");
    if (!g_have_launch_ms) return fail(TTN_ERR_ARG, "ttn_last_launch_ms: no ttn_dot / ttn_norm / ttn_orthogonalize / ttn_tto_mul / ttn_tto_decomp_dev launch yet");
    HIPCHK(hipEventSynchronize(g_launch_ev1));
    HIPCHK(hipEventElapsedTime(ms, g_launch_ev0, g_launch_ev1));
    return TTN_OK;
}

int ttn_norm(ttn_tt_t a, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (a && out && a->el == 2) {               // norm = sqrt(max(real(dot(a, a)), 0))
        std::vector<double> z(2 * (size_t)a->batch);
        const int rcz = ttn_dot(a, a, z.data());
        if (rcz) return rcz;
        for (int b = 0; b < a->batch; ++b) out[b] = std::sqrt(std::max(z[2 * b], 0.0));
        return TTN_OK;
    }
    int rc = ttn_dot(a, a, out);
    if (rc) return rc;
    for (int b = 0; b < a->batch; ++b) { double v = out[b]; v = v < 0 ? 0.0 : v; out[b] = std::sqrt(v); }
    return TTN_OK;
}

int ttn_orthogonalize(ttn_tt_t x, int64_t center, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_orthogonalize", {x, y});
    if (!x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_orthogonalize: output must not alias the input");
    const int d = x->d;
    if (center < 1 || center > d) return fail(TTN_ERR_CENTER, "Impossible orthogonalization");
    // y ranks start from r_and_d_to_rks(x.rks, dims) but a left QR step sets r_{j+1} = min(rows, cols), which can
    // exceed that cap (the reference reassigns the rank, tt_tools.jl:522); they never exceed x's own ranks.
    std::vector<int64_t> yb(x->bound);
    for (int m = 0; m <= d; ++m) if (y->cap[m] < yb[m]) return fail(TTN_ERR_CAPACITY, "ttn_orthogonalize: destination capacity too small");
    long long rmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) rmax = std::max<long long>(rmax, x->bound[m]);
    for (int k = 0; k < d; ++k) nmax = std::max<long long>(nmax, x->dims[k]);
    const long long mm = nmax * rmax;           // rows of the tall matrices
    const long long per_train = 2 * mm * rmax + 4 * rmax * rmax + 2 * QR_NB * mm + ((rmax + QR_NB - 1) / QR_NB) * QR_NB * QR_NB + 64   // Tm, Qb, 4 R, Vb, Wb, T panels
                                + 3 * 128 * 128;                                                                                  // Gram matrices / L1 of the Cholesky-QR steps
    int rc = scratch_take(sizeof(double) * (size_t)per_train * x->batch + sizeof(int) * (5 * (size_t)x->batch + 16) + 64);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * x->batch);
    if (rc) return rc;
    OrthoArgs P;
    P.x = x->dev(); P.y = y->dev();
    P.center = (int)center - 1;
    P.scratch = g_scratch.as<double>(); P.scratch_stride = per_train;
    P.mmax = (int)mm; P.rmax = (int)rmax;
    { const char* e = getenv("TTN_ORTHO_CHOLQR"); P.no_cholqr = (e && atoi(e) == 1) ? 2 : 0; }
    // Rank <= 64 QTT trains: the ramp sites at the right end by one wave per train (csrc/ttn_ortho_ramp.h), the tall sites and the
    // centre core by the 512-thread kernel (two workgroups per CU, csrc/ttn_ortho512.h), the 1024-thread kernel before them for the
    // left sweep and after them only for the trains they did not finish.  Measured against the single launch (d = 30, rank 64, centre
    // 1): 1.24 vs 1.28 ms for one train, 1.28 vs 1.48 at 8, 1.41 vs 1.89 at 256, 3.36 vs 6.89 at 1024.  TTN_ORTHO512 = 0 / 1 forbids /
    // forces it.
    bool use512 = nmax == 2 && rmax <= 64 && d <= TTN_MAX_D * 8 && center < d;
    for (int k = 0; k < d; ++k) use512 = use512 && x->dims[k] == 2;
    { const char* e = getenv("TTN_ORTHO512"); if (e) use512 = atoi(e) != 0 && nmax == 2 && rmax <= 64 && d <= TTN_MAX_D * 8; }
    P.mode = 0; P.trains = nullptr;
    g_ortho_state_off = sizeof(double) * (size_t)per_train * x->batch;
    g_ortho_state_batch = x->batch;
    P.state = reinterpret_cast<int*>(g_scratch.as<char>() + g_ortho_state_off);
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    if (use512) {
        P.mode = 1;
        int* left = P.state + 4 * (size_t)x->batch;                            // count, then the list of trains k_ortho512 did not finish
        HIPCHK(hipMemsetAsync(left, 0, sizeof(int), g_stream));
        // the ramp sites at the right end (wide / square LQ steps) go to one wave per train (csrc/ttn_ortho_ramp.h); the 1024-thread
        // kernel then only runs the left sweep, and not at all when the centre is the first site.
        if (P.center > 0) hipLaunchKernelGGL(k_orthogonalize, dim3(x->batch), dim3(TTN_WG), ORTHO_LDS_BYTES, g_stream, P);
        P.mode = P.center > 0 ? 4 : 5;
        hipLaunchKernelGGL(k_ortho_ramp, dim3((x->batch + ORAMP_WG / 64 - 1) / (ORAMP_WG / 64)), dim3(ORAMP_WG), 0, g_stream, P, (int)x->batch);
        hipLaunchKernelGGL(k_ortho512, dim3(x->batch), dim3(O5_WG), O5_LDS_BYTES(d), g_stream, P);
        // the 512-thread kernel finishes a train (centre core included) unless it had to stop — a refused step, a site outside its
        // class: the third launch takes only those trains (1024 heavy workgroups cost 4 ms of dispatch even when they do nothing)
        int h_left = 0;
        HIPCHK(hipMemcpyAsync(&h_left, left, sizeof(int), hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        if (h_left > 0) {
            P.mode = 3;
            P.trains = left + 1;
            hipLaunchKernelGGL(k_orthogonalize, dim3(h_left), dim3(TTN_WG), ORTHO_LDS_BYTES, g_stream, P);
        }
    } else {
        hipLaunchKernelGGL(k_orthogonalize, dim3(x->batch), dim3(TTN_WG), ORTHO_LDS_BYTES, g_stream, P);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    y->bound = yb;
    for (int b = 0; b < y->batch; ++b)
        for (int k = 0; k < d; ++k) y->ot[(size_t)b * d + k] = (k < center - 1) ? 1 : (k > center - 1 ? -1 : 0);
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_DOT_H
