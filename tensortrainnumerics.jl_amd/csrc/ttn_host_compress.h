// ttn_host_compress.h — host API: tt_compress and what goes with it.
// Rank bounds, the compress launch in its two builds, bond truncation, sweeps; the boundary-core hand-off and the fused apply of core-wise
// sharded chains; the status queries; the singular-value capture.  Owns g_next_train, the train counter of the persistent grid, which
// ttn_init allocates.
// ttn_status_all / ttn_compress_status stand here because what they report is what the dense kernels, k_compress first, record on a handle (they fold
// it with k_fold_status and walk g_live, both of ttn_host_core.h).  ttn_stream_handle only hands out g_stream; it stands with the
// boundary-core hand-off it was added for (include/ttn.h declares it there), which orders the caller's streams against the library's.
#ifndef TTN_HOST_COMPRESS_H
#define TTN_HOST_COMPRESS_H
#include "ttn_host_core.h"
#include "ttn_host_stream.h"
#include "ttn_wg512.h"
#include "ttn_dense_kernels.h"
#include "ttn_cplx_kernels.h"

extern "C" {
// ---- tt_compress: rank bounds, the launch, bond truncation, sweeps ---------------------------------------------------------------------
// Upper bounds on the ranks during / after tt_compress! (or one _tt_bond_truncate!).  The reference sets
// r = min(length(s), max_bond) with length(s) = min(n_k r_{k-1}, n_{k+1} r_{k+1}) (tt_cross_interpolation.jl:152,164),
// so a bond rank can GROW when it was below both of those (rank-deficient input).  need[m] = largest rank bond m can
// take at any time (buffers / handle capacity must hold it), fin[m] = bound after the call.
static void rank_bounds(int d, const int64_t* dims, const int64_t* rks, int64_t max_bond, int64_t sweeps, int64_t k_single,
                        std::vector<int64_t>& need, std::vector<int64_t>& fin, long long& pmax, long long& qmax,
                        int64_t k_first = 0, int64_t k_last = 0 /* 0-based bond range when k_single < 0 */) {
    fin.assign(rks, rks + d + 1);
    need = fin;
    pmax = 1; qmax = 1;
    auto stepk = [&](int k) {      // 0-based bond between cores k, k+1
        const long long mr = dims[k] * fin[k], mc = dims[k + 1] * fin[k + 2];
        const long long p = std::min(mr, mc), q = std::max(mr, mc);
        pmax = std::max(pmax, p); qmax = std::max(qmax, q);
        fin[k + 1] = std::min<long long>(p, max_bond);
        need[k + 1] = std::max(need[k + 1], fin[k + 1]);
    };
    if (k_single > 0) { stepk((int)k_single - 1); return; }
    if (k_single < 0) {
        if (k_first <= k_last) { for (int64_t k = k_first; k <= k_last; ++k) stepk((int)k); }
        else { for (int64_t k = k_first; k >= k_last; --k) stepk((int)k); }
        return;
    }
    for (int64_t sw = 0; sw < sweeps; ++sw) {
        for (int k = 0; k + 1 < d; ++k) stepk(k);
        for (int k = d - 2; k >= 0; --k) stepk(k);
    }
}

int ttn_compress_rank_bound(int64_t d, const int64_t* dims, const int64_t* rks, int64_t max_bond, int64_t sweeps, int64_t k,
                            int64_t* need_out, int64_t* final_out) {
    if (!dims || !rks || d < 1 || max_bond < 1 || sweeps < 1 || k < 0 || k > d - 1)
        return fail(TTN_ERR_ARG, "bad argument");
    std::vector<int64_t> need, fin;
    long long pm, qm;
    rank_bounds((int)d, dims, rks, max_bond, sweeps, k, need, fin, pm, qm);
    for (int64_t m = 0; m <= d; ++m) { if (need_out) need_out[m] = need[m]; if (final_out) final_out[m] = fin[m]; }
    return TTN_OK;
}

static DevBuf g_next_train;       // train counter of the persistent k_compress grid
// Which build runs a compress launch, and on how many workgroup slots.  More trains than CUs: the 512-thread build on a PERSISTENT
// grid of two workgroups per CU that pull trains from a counter (scratch per slot); otherwise one 1024-thread workgroup per train
// (lowest latency for a single train).  TTN_WG512=1 / 0 forces / forbids the 512-thread build (diagnostics, parity tests).
#define TTN_NUM_CUS 256
static bool compress_use_wg512(int batch) {
    const char* e = getenv("TTN_WG512");
    if (e) return atoi(e) != 0;
    return batch > TTN_NUM_CUS;
}
static int compress_slots(int batch) { return compress_use_wg512(batch) ? std::min(batch, 2 * TTN_NUM_CUS) : batch; }

// Limits of k_zcompress (include/ttn.h): short side <= 512, long side <= 8192 complex
#define TTN_ZC_PMAX 512
#define TTN_ZC_QMAX 8192
// Everything that can refuse a compress launch — capacity of the handle for the ranks the sweep can reach from `bound`, the size
// limits of the merged matrices, the scratch allocation — checked WITHOUT touching the handle (ttn_apply_compress runs this on the
// product's ranks before it overwrites y's).
// The two element types differ in those limits and in the scratch of a train (per_train, in doubles).
static int compress_precheck(ttn_tt_t psi, const std::vector<int64_t>& bound, int64_t k_single, int64_t max_bond, int64_t sweeps,
                             int64_t k_first, int64_t k_last, std::vector<int64_t>& fin, long long& pmax, long long& qmax, long long& per_train) {
    const int d = psi->d;
    std::vector<int64_t> need;
    pmax = 1; qmax = 1;
    rank_bounds(d, psi->dims.data(), bound.data(), max_bond, sweeps, k_single, need, fin, pmax, qmax, k_first, k_last);
    for (int m = 0; m <= d; ++m)
        if (need[m] > psi->cap[m]) return fail(TTN_ERR_CAPACITY, "ttn_compress: a bond rank can grow beyond the handle's capacity (see ttn_compress_rank_bound)");
    if (psi->el == 2) {                        // k_zcompress: one workgroup per train
        if (pmax > TTN_ZC_PMAX || qmax > TTN_ZC_QMAX) return fail(TTN_ERR_UNSUPPORTED, "ttn_compress (ComplexF64): merged matrix larger than 512 x 8192");
        per_train = zcompress_scratch(pmax, qmax);
        return scratch_take(sizeof(double) * (size_t)per_train * psi->batch);
    }
    if (pmax > 4096 || qmax > 16384) return fail(TTN_ERR_UNSUPPORTED, "ttn_compress: merged matrix larger than 4096 x 16384");
    per_train = 2 * pmax * qmax + QR_NB * qmax + pmax * QR_NB + 2 * pmax * pmax + 4 * pmax + 64 + 6 * 128 * 128;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * compress_slots(psi->batch));
    if (rc) return rc;
    return g_dout.ensure(sizeof(double) * psi->batch);
}

static int launch_compress(ttn_tt_t psi, int64_t k_single, int64_t max_bond, double truncerr, int64_t sweeps,
                           int64_t k_first = 0, int64_t k_last = 0, ttn_tto_t fuseA = nullptr, ttn_tt_t fusex = nullptr, int fused_first_real = 0) {
    const int d = psi->d;
    if (d < 2 && k_single == 0) return TTN_OK;
    std::vector<int64_t> fin;
    long long pmax = 1, qmax = 1, per_train = 0;
    int rc = compress_precheck(psi, psi->bound, k_single, max_bond, sweeps, k_first, k_last, fin, pmax, qmax, per_train);
    if (rc) return rc;
    if (psi->el == 2) {                        // ComplexF64: k_zcompress (no fused merge, no singular-value capture, no 512-thread build)
        ZCompressArgs P;
        P.tt = psi->dev();
        P.max_bond = max_bond; P.truncerr = truncerr; P.sweeps = (int)sweeps;
        P.k_single = (int)k_single; P.k_first = (int)k_first; P.k_last = (int)k_last;
        P.scratch = g_scratch.as<double>();
        P.scratch_stride = per_train;
        P.pmax = (int)pmax; P.qmax = (int)qmax;
        P.status = psi->d_status;
        P.sweep_stats = psi->d_status + psi->batch;
        hipLaunchKernelGGL(k_zcompress, dim3(psi->batch), dim3(TTN_ZC_WG), TTN_ZC_LDS_BYTES, g_stream, P);
        HIPCHK(hipGetLastError());
        psi->bound = fin;
        return TTN_OK;
    }
    const int steps = k_single > 0 ? 1 : (k_single < 0 ? (int)(std::llabs(k_last - k_first) + 1) : (int)(2 * (d - 1) * sweeps));
    if (psi->sv_on) {
        if (psi->sv_steps < steps || psi->sv_pmax < pmax) {
            if (psi->d_sv) { HIPCHK(hipStreamSynchronize(g_stream)); HIPCHK(hipFree(psi->d_sv)); psi->d_sv = nullptr; }
            HIPCHK(hipMalloc((void**)&psi->d_sv, sizeof(double) * (size_t)psi->batch * steps * pmax));
        }
        psi->sv_steps = steps;
        psi->sv_pmax = (int)pmax;
    }
    CompressArgs P;
    P.tt = psi->dev();
    P.max_bond = max_bond;
    P.truncerr = truncerr;
    P.sweeps = (int)sweeps;
    P.k_single = (int)k_single;
    P.k_first = (int)k_first; P.k_last = (int)k_last;
    P.scratch = g_scratch.as<double>();
    P.scratch_stride = per_train;
    P.pmax = (int)pmax; P.qmax = (int)qmax;
    P.sv_out = psi->sv_on ? psi->d_sv : nullptr;
    P.sv_steps = steps;
    P.status = psi->d_status;
    P.sweep_stats = psi->d_status + psi->batch;
    P.rank_rule = 0;
    P.fused = (fuseA && fusex) ? 1 : 0;
    P.fused_first_real = fused_first_real;
    if (P.fused) { P.op = fuseA->dev(); P.x = fusex->dev(); }
    else { memset(&P.op, 0, sizeof(P.op)); memset(&P.x, 0, sizeof(P.x)); }
    { const char* e = getenv("TTN_FAST"); P.fast = e ? atoi(e) : 1; }
    if (compress_use_wg512(psi->batch)) {
        HIPCHK(hipMemsetAsync(g_next_train.p, 0, sizeof(int), g_stream));
        P.next_train = g_next_train.as<int>();
        const int rc512 = ttn_wg512_launch_compress(&P, sizeof(P), compress_slots(psi->batch), g_stream);
        if (rc512) return hipfail((hipError_t)rc512, "k_compress (512-thread build)");
    } else {
        P.next_train = nullptr;
        hipLaunchKernelGGL(k_compress, dim3(psi->batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, P);
        HIPCHK(hipGetLastError());
    }
    psi->bound = fin;
    return TTN_OK;
}

int ttn_compress(ttn_tt_t psi, int64_t max_bond, double truncerr, int64_t sweeps) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!psi) return fail(TTN_ERR_ARG, "null handle");
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    return launch_compress(psi, 0, max_bond, truncerr, sweeps);
}

int ttn_bond_truncate(ttn_tt_t psi, int64_t k, int64_t max_bond, double truncerr) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!psi) return fail(TTN_ERR_ARG, "null handle");
    if (k < 1 || k >= psi->d) return fail(TTN_ERR_BOND_INDEX, "k must be in 1:(N-1)");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    return launch_compress(psi, k, max_bond, truncerr, 1);
}

int ttn_sweep(ttn_tt_t psi, int64_t k_first, int64_t k_last, int64_t max_bond, double truncerr) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!psi) return fail(TTN_ERR_ARG, "null handle");
    if (k_first < 1 || k_first >= psi->d || k_last < 1 || k_last >= psi->d) return fail(TTN_ERR_BOND_INDEX, "k must be in 1:(N-1)");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    return launch_compress(psi, -1, max_bond, truncerr, 1, k_first - 1, k_last - 1);
}

// ---- boundary-core hand-off of core-wise sharded chains --------------------------------------------
// A core is stored compactly (current ranks) at the start of its slot, so the first dims[k]*bound[k]*bound[k+1] doubles
// of every train's slot carry it; they move to / from a dense [batch][that many] device buffer with one 2-D copy.
int ttn_tt_core_extent(ttn_tt_t h, int64_t k, int64_t* doubles_per_train, int64_t* bound_left, int64_t* bound_right) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    F64_ONLY("ttn_tt_core_extent", {h});
    if (!h || k < 1 || k > h->d) return fail(TTN_ERR_ARG, "bad core index");
    const int64_t bl = h->bound[k - 1], br = h->bound[k];
    if (doubles_per_train) *doubles_per_train = h->dims[k - 1] * bl * br;
    if (bound_left) *bound_left = bl;
    if (bound_right) *bound_right = br;
    return TTN_OK;
}

int ttn_tt_core_export(ttn_tt_t h, int64_t k, double* dev_buf, int64_t* dev_rks2) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_core_export", {h});
    if (!h || !dev_buf || !dev_rks2 || k < 1 || k > h->d) return fail(TTN_ERR_ARG, "bad argument");
    const size_t w = sizeof(double) * (size_t)(h->dims[k - 1] * h->bound[k - 1] * h->bound[k]);
    HIPCHK(hipMemcpy2DAsync(dev_buf, w, h->d_data + h->off[k - 1], sizeof(double) * (size_t)h->stride, w, h->batch,
                            hipMemcpyDeviceToDevice, g_stream));
    HIPCHK(hipMemcpy2DAsync(dev_rks2, 2 * sizeof(long long), h->d_rks + (k - 1), sizeof(long long) * (size_t)(h->d + 1),
                            2 * sizeof(long long), h->batch, hipMemcpyDeviceToDevice, g_stream));
    return TTN_OK;
}

int ttn_tt_core_import(ttn_tt_t h, int64_t k, const double* dev_buf, const int64_t* dev_rks2, int64_t bound_left, int64_t bound_right) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_core_import", {h});
    if (!h || !dev_buf || !dev_rks2 || k < 1 || k > h->d || bound_left < 1 || bound_right < 1) return fail(TTN_ERR_ARG, "bad argument");
    if (bound_left > h->cap[k - 1] || bound_right > h->cap[k]) return fail(TTN_ERR_CAPACITY, "ttn_tt_core_import: core does not fit the slot");
    const size_t w = sizeof(double) * (size_t)(h->dims[k - 1] * bound_left * bound_right);
    HIPCHK(hipMemcpy2DAsync(h->d_data + h->off[k - 1], sizeof(double) * (size_t)h->stride, dev_buf, w, w, h->batch,
                            hipMemcpyDeviceToDevice, g_stream));
    HIPCHK(hipMemcpy2DAsync(h->d_rks + (k - 1), sizeof(long long) * (size_t)(h->d + 1), dev_rks2, 2 * sizeof(long long),
                            2 * sizeof(long long), h->batch, hipMemcpyDeviceToDevice, g_stream));
    h->bound[k - 1] = bound_left;
    h->bound[k] = bound_right;
    return TTN_OK;
}

int ttn_apply_compress(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y, int64_t max_bond, double truncerr, int64_t sweeps) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    if (!A || !x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    if (int rb = single_op(A, "ttn_apply_compress")) return rb;
    const bool cplx = A->el == 2 || x->el == 2 || y->el == 2;     // ComplexF64: apply, then round (no fused complex merge)
    const char* nf = getenv("TTN_NOFUSE");
    if (!cplx && (x->d < 2 || (nf && atoi(nf)))) {          // nothing to fuse into / diagnostic switch
        int rc = ttn_apply(A, x, y);
        if (rc) return rc;
        return ttn_compress(y, max_bond, truncerr, sweeps);
    }
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (cplx) {
        if (y->el != 2 || (A->el != 2 && x->el != 2)) return refuse_mixed("ttn_apply_compress");
    } else {
        if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
        if (x == y) return fail(TTN_ERR_ARG, "ttn_apply_compress: output must not alias the input");
    }
    const int d = x->d;
    int rc = apply_capacity(A, x, y);
    if (rc) return rc;
    // every check that can refuse the rounding runs on the product's ranks BEFORE y is touched: on an error return y still holds
    // what it held (ranks, bounds, gauge flags and cores)
    std::vector<int64_t> yb(d + 1), fin_;
    for (int m = 0; m <= d; ++m) yb[m] = A->rks[m] * x->bound[m];
    // (the workspace is taken here for its size alone — launch_compress takes it again, nothing is in it in between)
    if (d >= 2) { long long pm_, qm_, pt_; if ((rc = compress_precheck(y, yb, 0, max_bond, sweeps, 0, 0, fin_, pm_, qm_, pt_))) return rc; }
    if (cplx) {
        if ((rc = ttn_apply(A, x, y))) return rc;
        return ttn_compress(y, max_bond, truncerr, sweeps);
    }
    // FUSED: y = A*x is never written to HBM.  y only receives its ranks (A.rks .* x.rks, tt_operations.jl:103); the first
    // L->R sweep of k_compress builds each merged matrix straight from core k of y, x_{k+1} and A_{k+1}.
    if ((rc = apply_ranks(A, x, y))) return rc;
    return launch_compress(y, 0, max_bond, truncerr, sweeps, 0, 0, A, x);
}

// ---- fused apply for core-wise sharded chains: the product's ranks first, then ONE L->R pass over a bond range whose right cores
// are still virtual.  Between the two calls a boundary core may be imported into y (ttn_tt_core_import).
int ttn_apply_begin(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_apply_begin", {x, y}, {A});
    if (!A || !x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (int rb = single_op(A, "ttn_apply_begin")) return rb;
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_apply_begin: output must not alias the input");
    const int rc = apply_capacity(A, x, y);
    return rc ? rc : apply_ranks(A, x, y);
}

int ttn_apply_sweep(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y, int64_t k_first, int64_t k_last, int64_t max_bond, double truncerr, int first_core_real) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_apply_sweep", {x, y}, {A});
    if (!A || !x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (int rb = single_op(A, "ttn_apply_sweep")) return rb;
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (k_first < 1 || k_first >= y->d || k_last < k_first || k_last >= y->d) return fail(TTN_ERR_BOND_INDEX, "ttn_apply_sweep: need 1 <= k_first <= k_last <= N-1 (one L->R pass)");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    return launch_compress(y, -1, max_bond, truncerr, 1, k_first - 1, k_last - 1, A, x, first_core_real ? 1 : 0);
}

// The HIP stream every call of this library is enqueued on (hipStream_t): lets a caller order its own streams against the
// library's work with events instead of host synchronisation (the boundary-core hand-offs of pipeline.py)
int ttn_stream_handle(void** stream) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!stream) return fail(TTN_ERR_ARG, "null pointer");
    *stream = (void*)g_stream;
    return TTN_OK;
}

int ttn_status_all(void) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    unsigned seen = 0;
    for (ttn_tt_s* h : g_live)
        if (h->d_status) hipLaunchKernelGGL(k_fold_status, dim3(1), dim3(64), 0, g_stream, (const int*)h->d_status, h->batch, g_pending_status.as<unsigned>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&seen, g_pending_status.p, sizeof(unsigned), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemsetAsync(g_pending_status.p, 0, sizeof(unsigned), g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return status_error(seen);
}

int ttn_compress_status(ttn_tt_t psi, int64_t* total_jacobi_sweeps) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!psi) return fail(TTN_ERR_ARG, "null handle");
    if (total_jacobi_sweeps) {
        std::vector<int> st(psi->batch);
        HIPCHK(hipMemcpyAsync(st.data(), psi->d_status + psi->batch, sizeof(int) * psi->batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        for (int b = 0; b < psi->batch; ++b) total_jacobi_sweeps[b] = st[b];
    }
    unsigned seen = 0;
    const int rc = take_status(psi, seen);
    return rc ? rc : status_error(seen);
}

// ---- singular-value capture -----------------------------------------------------------------------
int ttn_sv_capture(ttn_tt_t h, int enable) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    F64_ONLY("ttn_sv_capture", {h});
    if (!h) return fail(TTN_ERR_ARG, "null handle");
    h->sv_on = enable != 0;
    return TTN_OK;
}
int ttn_sv_get(ttn_tt_t h, int64_t b, int64_t step, double* out, int64_t cap, int64_t* n) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || !out || !n || b < 0 || b >= h->batch) return fail(TTN_ERR_ARG, "bad argument");
    if (!h->d_sv || step < 0 || step >= h->sv_steps) return fail(TTN_ERR_ARG, "no captured singular values for that step");
    std::vector<double> tmp(h->sv_pmax);
    HIPCHK(hipMemcpyAsync(tmp.data(), h->d_sv + ((size_t)b * h->sv_steps + step) * h->sv_pmax, sizeof(double) * h->sv_pmax, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    int64_t cnt = 0;
    for (int i = 0; i < h->sv_pmax && tmp[i] >= 0.0; ++i) { if (cnt < cap) out[cnt] = tmp[i]; ++cnt; }
    *n = std::min(cnt, cap);
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_COMPRESS_H
