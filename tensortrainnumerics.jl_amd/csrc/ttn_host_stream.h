// ttn_host_stream.h — host API: the streaming operations: apply, hadamard, add, the scale family, apply_axpby.
// g_grad_coef stands here with ttn_apply_axpby, the lowest of its users; the core gradients (ttn_dot_pullback, ttn_tt_cores_axpby) are the
// other.  stream_grid, scaled_core, launch_scale and launch_add serve the features above as well.
#ifndef TTN_HOST_STREAM_H
#define TTN_HOST_STREAM_H
#include "ttn_host_core.h"
#include "ttn_host_handles.h"
#include "ttn_stream_kernels.h"
#include "ttn_cplx_kernels.h"
#include "ttn_step_kernels.h"

extern "C" {
// ---- streaming ops --------------------------------------------------------------------------------
static dim3 stream_grid(long long max_items, int d, int batch) {
    long long gx = (max_items + TTN_STREAM_TB - 1) / TTN_STREAM_TB;
    gx = std::max<long long>(1, std::min<long long>(gx, 4096));
    return dim3((unsigned)gx, (unsigned)d, (unsigned)batch);
}

// The two steps every form of A * x shares (ttn_apply, ttn_apply_compress, ttn_apply_begin).  apply_capacity: y can hold the product's
// ranks A.rks .* x.rks.  apply_ranks: y receives them, on the device and as host bounds, with the gauge flags of zeros_tt
// (tt_operations.jl:103).
static int apply_capacity(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y) {
    for (int m = 0; m <= x->d; ++m) if (y->cap[m] < A->rks[m] * x->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_apply: destination capacity too small");
    return TTN_OK;
}
static int apply_ranks(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y) {
    hipLaunchKernelGGL(k_ranks_mul_op, dim3(x->batch), dim3(64), 0, g_stream, y->dev(), A->dev(), x->dev());
    HIPCHK(hipGetLastError());
    for (int m = 0; m <= x->d; ++m) y->bound[m] = A->rks[m] * x->bound[m];
    std::fill(y->ot.begin(), y->ot.end(), 0);
    return TTN_OK;
}

// Float64 operator and trains: k_apply.  A complex operator and / or a complex train into a complex y: k_zapply.
int ttn_apply(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_apply: output must not alias the input");
    if (int rb = op_batch_fits(A, x->batch)) return rb;
    const bool cplx = A->el == 2 || x->el == 2 || y->el == 2;
    if (cplx) { if (int rb = single_op(A, "ttn_apply (ComplexF64)")) return rb; }
    if (cplx && y->el != 2) return refuse_mixed("ttn_apply (a complex operand needs a ComplexF64 output handle)");
    if (cplx && A->el != 2 && x->el != 2) return refuse_mixed("ttn_apply (a ComplexF64 output needs a complex operator or train)");
    const int d = x->d;
    int rc = apply_capacity(A, x, y);
    if (rc) return rc;
    const dim3 tb(TTN_STREAM_TB);
    if (cplx) {
        long long items = 1;
        for (int k = 0; k < d; ++k) {
            const long long P = (long long)A->rks[k] * x->bound[k], Q = (long long)A->rks[k + 1] * x->bound[k + 1];
            if (stream_fibres_too_many(P * Q)) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply: 2^31 or more fibres in one output core (32-bit element indices)");
            items = std::max(items, P * ((Q + TTN_ZAPPLY_K - 1) / TTN_ZAPPLY_K));
        }
        if ((rc = apply_ranks(A, x, y))) return rc;
        const dim3 grid = stream_grid(items, d, x->batch);
        if (A->el == 2 && x->el == 2) hipLaunchKernelGGL((k_zapply<true, true>), grid, tb, 0, g_stream, A->dev(), x->dev(), y->dev());
        else if (A->el == 2) hipLaunchKernelGGL((k_zapply<true, false>), grid, tb, 0, g_stream, A->dev(), x->dev(), y->dev());
        else hipLaunchKernelGGL((k_zapply<false, true>), grid, tb, 0, g_stream, A->dev(), x->dev(), y->dev());
    } else {
        long long maxfib = 0;
        for (int k = 0; k < d; ++k) maxfib = std::max<long long>(maxfib, (long long)x->bound[k] * x->bound[k + 1]);
        if (stream_fibres_too_many(maxfib * std::max<long long>(1, A->rks[0]))) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply: 2^31 or more fibres in one core (32-bit element indices)");
        for (int k = 0; k < d; ++k) if (stream_fibres_too_many((long long)y->cap[k] * y->cap[k + 1])) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply: 2^31 or more fibres in one output core (32-bit element indices)");
        if ((rc = apply_ranks(A, x, y))) return rc;
        // LDS of k_apply: the largest operator core (if it fits TTN_APPLY_LDS_DOUBLES) + the store-transpose buffer for the largest left rank
        long long amax_ = 0, rlmax_ = 1;
        for (int k = 0; k < d; ++k) { amax_ = std::max<long long>(amax_, (long long)A->dims[k] * A->dims[k] * A->rks[k] * A->rks[k + 1]); rlmax_ = std::max<long long>(rlmax_, A->rks[k]); }
        const int lds_a = amax_ <= TTN_APPLY_LDS_DOUBLES ? (int)amax_ : 0;
        const int lds_rl = rlmax_ <= TTN_APPLY_MAX_RL ? (int)rlmax_ : 0;
        const size_t apply_lds = sizeof(double) * (size_t)((lds_a + 1) & ~1) + sizeof(double) * 2 * (size_t)(TTN_STREAM_TB / 64) * lds_rl * 64;
        // grid: output rows x groups of TTN_APPLY_K output columns when every site has n = 2 and the operator cores fit the LDS (the mapping
        // of k_apply's fast path), input fibres otherwise
        long long apply_items = maxfib;
        {
            bool qtt = lds_a > 0;
            for (int k = 0; k < d; ++k) qtt = qtt && x->dims[k] == 2;
            if (qtt) {
                apply_items = 0;
                for (int k = 0; k < d; ++k)
                    apply_items = std::max<long long>(apply_items, (long long)A->rks[k] * x->bound[k] * (((long long)A->rks[k + 1] * x->bound[k + 1] + TTN_APPLY_K - 1) / TTN_APPLY_K));
            }
        }
        hipLaunchKernelGGL(k_apply, stream_grid(apply_items, d, x->batch), tb, apply_lds, g_stream, A->dev(), x->dev(), y->dev(), lds_a, lds_rl);
    }
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_hadamard(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y || !z) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || !same_dims(x->dims, z->dims)) return fail(TTN_ERR_DIMS, "Incompatible TT dimensions");
    if (x->batch != y->batch || x->batch != z->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (z == x || z == y) return fail(TTN_ERR_ARG, "ttn_hadamard: output must not alias an input");
    if (x->el != y->el || x->el != z->el) return refuse_mixed("ttn_hadamard");
    const int d = x->d;
    long long maxpq = 0;
    for (int m = 0; m <= d; ++m) if (z->cap[m] < x->bound[m] * y->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_hadamard: destination capacity too small");
    for (int k = 0; k < d; ++k) maxpq = std::max<long long>(maxpq, (long long)x->bound[k] * y->bound[k] * x->bound[k + 1] * y->bound[k + 1]);
    if (stream_fibres_too_many(maxpq)) return fail(TTN_ERR_UNSUPPORTED, "ttn_hadamard: 2^31 or more fibres in one core (32-bit element indices)");
    hipLaunchKernelGGL(k_ranks_mul, dim3(x->batch), dim3(64), 0, g_stream, z->dev(), x->dev(), y->dev());
    bool qtt = true;
    for (int k = 0; k < d; ++k) qtt = qtt && x->dims[k] == 2;
    if (x->el == 2) hipLaunchKernelGGL(k_zhadamard, stream_grid((maxpq + TTN_ZHAD_K - 1) / TTN_ZHAD_K, d, x->batch), dim3(TTN_STREAM_TB), 0, g_stream, x->dev(), y->dev(), z->dev());
    else
    hipLaunchKernelGGL(k_hadamard, stream_grid(qtt ? (maxpq + TTN_HAD_K - 1) / TTN_HAD_K : maxpq, d, x->batch), dim3(TTN_STREAM_TB), 0, g_stream, x->dev(), y->dev(), z->dev());
    HIPCHK(hipGetLastError());
    for (int m = 0; m <= d; ++m) z->bound[m] = x->bound[m] * y->bound[m];
    std::fill(z->ot.begin(), z->ot.end(), 0);
    return TTN_OK;
}

// The largest number of fibres r_k r_{k+1} of a core with ranks r, and the k_add launch z = x + y for result ranks zr.  n2: every
// physical dimension of the trains as k_add reads them is 2 (its mapping of TTN_ADD_K fibres per thread), one fibre per thread otherwise.
static long long max_fibres(const std::vector<int64_t>& r) {
    long long m = 0;
    for (size_t k = 0; k + 1 < r.size(); ++k) m = std::max<long long>(m, (long long)r[k] * r[k + 1]);
    return m;
}
static void launch_add(const TTDev& x, const TTDev& y, const TTDev& z, const std::vector<int64_t>& zr, bool n2, int batch) {
    const long long maxpq = max_fibres(zr);
    hipLaunchKernelGGL(k_add, stream_grid(n2 ? (maxpq + TTN_ADD_K - 1) / TTN_ADD_K : maxpq, (int)zr.size() - 1, batch), dim3(TTN_STREAM_TB), 0, g_stream, x, y, z);
}

int ttn_add(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y || !z) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || !same_dims(x->dims, z->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch || x->batch != z->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (z == x || z == y) return fail(TTN_ERR_ARG, "ttn_add: output must not alias an input");
    if (x->el != y->el || x->el != z->el) return refuse_mixed("ttn_add");
    const int d = x->d;
    if (d < 2) return fail(TTN_ERR_UNSUPPORTED, "ttn_add: the reference's + is only defined for d >= 2");
    std::vector<int64_t> zb(d + 1);
    for (int m = 0; m <= d; ++m) zb[m] = (m == 0 || m == d) ? 1 : x->bound[m] + y->bound[m];
    for (int m = 0; m <= d; ++m) if (z->cap[m] < zb[m]) return fail(TTN_ERR_CAPACITY, "ttn_add: destination capacity too small");
    if (stream_fibres_too_many(max_fibres(zb))) return fail(TTN_ERR_UNSUPPORTED, "ttn_add: 2^31 or more fibres in one core (32-bit element indices)");
    hipLaunchKernelGGL(k_ranks_add, dim3(x->batch), dim3(64), 0, g_stream, z->dev(), x->dev(), y->dev());
    // (a complex core (n, r, r') is byte for byte the real core (2n, r, r') and + only copies: k_add runs on that view)
    bool qtt = x->el == 1;
    for (int k = 0; k < d; ++k) qtt = qtt && x->dims[k] == 2;
    launch_add(x->dev(), y->dev(), z->dev(), zb, qtt, x->batch);
    HIPCHK(hipGetLastError());
    z->bound = zb;
    std::fill(z->ot.begin(), z->ot.end(), 0);
    return TTN_OK;
}

static DevBuf g_which;            // [batch] scaled core per train when the gauge flags differ (scaled_core)
// The core scalar multiplication scales: the first one with ot == 0, else the first (tt_operations.jl:262).  Uniform over the batch
// -> `which`; trains with different gauge flags (uploaded one by one, or zeroed by ttn_scale_batch) -> a per-train device table.
// ot: [batch][d] gauge flags.
static int scaled_core(const int64_t* ot, int d, int batch, int& which, const int*& which_b) {
    std::vector<int> h_which(batch, 0);
    bool uniform = true;
    for (int b = 0; b < batch; ++b) {
        for (int k = 0; k < d; ++k) if (ot[(size_t)b * d + k] == 0) { h_which[b] = k; break; }
        uniform = uniform && h_which[b] == h_which[0];
    }
    which = h_which[0];
    which_b = nullptr;
    if (uniform) return TTN_OK;
    const int rc = g_which.ensure(sizeof(int) * batch);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(g_which.p, h_which.data(), sizeof(int) * batch, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));              // h_which is a local
    which_b = g_which.as<int>();
    return TTN_OK;
}

// The launch of y = a * x on trains of element type `el` (an operator passes its vector view): k_scale with the factor ar, k_scale_batch
// with one factor per train (ab: device), k_zscale with the complex factor (ar, ai) or one per train (ab: device, interleaved).
// dims / rks: physical dimensions (in elements) and rank bounds of x; zero: the one factor is 0.
static void launch_scale(int el, int d, int batch, const int64_t* dims, const int64_t* rks, const TTDev& x, const TTDev& y, double ar, double ai,
                         const double* ab, int which, const int* which_b, bool zero) {
    long long maxsz = 0;
    for (int k = 0; k < d; ++k) maxsz = std::max<long long>(maxsz, (long long)dims[k] * rks[k] * rks[k + 1]);
    const dim3 tb(TTN_STREAM_TB);
    if (el == 2) hipLaunchKernelGGL(k_zscale, stream_grid((maxsz + 3) / 4, d, batch), tb, 0, g_stream, x, y, ar, ai, which, zero ? 1 : 0, which_b, ab);
    else if (ab) hipLaunchKernelGGL(k_scale_batch, stream_grid((maxsz + 7) / 8, d, batch), tb, 0, g_stream, x, y, ab, which, which_b);
    else hipLaunchKernelGGL(k_scale, stream_grid((maxsz + 7) / 8, d, batch), tb, 0, g_stream, x, y, ar, which, zero ? 1 : 0, which_b);
}

// y = a * x on handles of one element type, behind every exported scale of a train.  The factor is (ar, ai) (ai: ComplexF64 only), or,
// with a_b, one per train: `batch` host values of x's element type.
static int scale_impl(const char* who, double ar, double ai, const double* a_b, ttn_tt_t x, ttn_tt_t y) {
    const int d = x->d, el = x->el;
    for (int m = 0; m <= d; ++m) if (y->cap[m] < x->bound[m]) return fail(TTN_ERR_CAPACITY, (std::string(who) + ": destination capacity too small").c_str());
    if (a_b) {
        const int rc = g_dout.ensure(sizeof(double) * el * x->batch);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(g_dout.p, a_b, sizeof(double) * el * x->batch, hipMemcpyHostToDevice, g_stream));
    }
    // i = findfirst(==(0), ot), else 1  (tt_operations.jl:262), per train
    int which = 0;
    const int* which_b = nullptr;
    { int rc_ = scaled_core(x->ot.data(), d, x->batch, which, which_b); if (rc_) return rc_; }
    const bool zero = !a_b && ar == 0.0 && ai == 0.0;
    if (x != y) hipLaunchKernelGGL(k_ranks_copy, dim3(x->batch), dim3(64), 0, g_stream, y->dev(), x->dev());
    launch_scale(el, d, x->batch, x->dims.data(), x->bound.data(), x->dev(), y->dev(), ar, ai, a_b ? g_dout.as<const double>() : nullptr, which, which_b, zero);
    HIPCHK(hipGetLastError());
    if (a_b) HIPCHK(hipStreamSynchronize(g_stream));      // `a_b` is caller memory and g_dout is reused by ttn_dot
    y->bound = x->bound;
    if (zero) std::fill(y->ot.begin(), y->ot.end(), 0); else y->ot = x->ot;
    if (a_b)
        for (int b = 0; b < x->batch; ++b) {
            bool zero_b = true;
            for (int c = 0; c < el; ++c) zero_b = zero_b && a_b[(size_t)el * b + c] == 0.0;
            if (zero_b) for (int k = 0; k < d; ++k) y->ot[(size_t)b * d + k] = 0;
        }
    return TTN_OK;
}

int ttn_scale_c64(double re, double im, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->el != 2 || y->el != 2) return refuse_mixed("ttn_scale_c64 (both handles must be ComplexF64)");
    return scale_impl("ttn_scale_c64", re, im, nullptr, x, y);
}

int ttn_scale_batch_c64(const double* a, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!a || !x || !y) return fail(TTN_ERR_ARG, "null pointer");
    if (!same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->el != 2 || y->el != 2) return refuse_mixed("ttn_scale_batch_c64 (both handles must be ComplexF64)");
    return scale_impl("ttn_scale_batch_c64", 0.0, 0.0, a, x, y);
}

int ttn_scale(double a, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->el != y->el) return refuse_mixed("ttn_scale");
    return scale_impl("ttn_scale", a, 0.0, nullptr, x, y);
}

int ttn_scale_batch(const double* a, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!a || !x || !y) return fail(TTN_ERR_ARG, "null pointer");
    if (!same_dims(x->dims, y->dims) || x->batch != y->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    F64_ONLY("ttn_scale_batch (ComplexF64 handles: ttn_scale_batch_c64)", {x, y});
    return scale_impl("ttn_scale_batch", 0.0, 0.0, a, x, y);
}

static DevBuf g_grad_coef;        // [2][batch] doubles: Delta of ttn_dot_pullback, alpha and beta of ttn_tt_cores_axpby
// z = alpha x + beta (A y) (include/ttn_step.h): k_apply_axpby, one launch for ttn_apply -> ttn_scale_batch x 2 -> ttn_add.  Factors that
// are the same for every train travel as kernel arguments; only a pair that differs over the batch is uploaded (and waited for).
int ttn_apply_axpby(const double* alpha, ttn_tt_t x, const double* beta, ttn_tto_t A, ttn_tt_t y, ttn_tt_t z) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !x || !y || !z) return fail(TTN_ERR_ARG, "null handle");
    F64_ONLY("ttn_apply_axpby", {x, y, z}, {A});
    if (!same_dims(A->dims, y->dims) || !same_dims(x->dims, y->dims) || !same_dims(x->dims, z->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch || x->batch != z->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (z == x || z == y) return fail(TTN_ERR_ARG, "ttn_apply_axpby: output must not alias an input");
    if (int rb = op_batch_fits(A, x->batch)) return rb;
    const int d = x->d, batch = x->batch;
    if (d < 2) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply_axpby: the reference's + is only defined for d >= 2");
    std::vector<int64_t> zb(d + 1);
    for (int m = 0; m <= d; ++m) zb[m] = (m == 0 || m == d) ? 1 : x->bound[m] + A->rks[m] * y->bound[m];
    for (int m = 0; m <= d; ++m) if (z->cap[m] < zb[m]) return fail(TTN_ERR_CAPACITY, "ttn_apply_axpby: destination capacity too small");
    long long maxfib = 0;
    for (int k = 0; k < d; ++k) maxfib = std::max<long long>(maxfib, (long long)y->bound[k] * y->bound[k + 1]);
    if (stream_fibres_too_many(maxfib * std::max<long long>(1, A->rks[0])) || stream_fibres_too_many(max_fibres(zb)))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_apply_axpby: 2^31 or more fibres in one core (32-bit element indices)");
    bool uniform = true;
    for (int b = 1; b < batch; ++b) uniform = uniform && (!alpha || alpha[b] == alpha[0]) && (!beta || beta[b] == beta[0]);
    const double* d_ab = nullptr;
    if (!uniform) {
        std::vector<double> ab(2 * (size_t)batch, 1.0);
        for (int b = 0; b < batch; ++b) { if (alpha) ab[b] = alpha[b]; if (beta) ab[(size_t)batch + b] = beta[b]; }
        const int rc = g_grad_coef.ensure(sizeof(double) * 2 * batch);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(g_grad_coef.p, ab.data(), sizeof(double) * 2 * batch, hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));              // ab is a local
        d_ab = g_grad_coef.as<const double>();
    }
    int which = 0;
    const int* which_b = nullptr;
    { const int rc = scaled_core(x->ot.data(), d, batch, which, which_b); if (rc) return rc; }
    hipLaunchKernelGGL(k_ranks_axpby, dim3(batch), dim3(64), 0, g_stream, z->dev(), x->dev(), A->dev(), y->dev());
    // LDS: the largest operator core, if it fits the bound of k_apply; grid: rows x groups of TTN_AXPBY_K columns on binary sites,
    // fibres elsewhere
    long long amax_ = 0, items = 1;
    for (int k = 0; k < d; ++k) {
        amax_ = std::max<long long>(amax_, (long long)A->dims[k] * A->dims[k] * A->rks[k] * A->rks[k + 1]);
        items = std::max<long long>(items, x->dims[k] == 2 ? (long long)zb[k] * ((zb[k + 1] + TTN_AXPBY_K - 1) / TTN_AXPBY_K) : (long long)zb[k] * zb[k + 1]);
    }
    const int lds_a = amax_ <= TTN_APPLY_LDS_DOUBLES ? (int)amax_ : 0;
    hipLaunchKernelGGL(k_apply_axpby, stream_grid(items, d, batch), dim3(TTN_STREAM_TB), sizeof(double) * (size_t)lds_a, g_stream, A->dev(), x->dev(), y->dev(),
                       z->dev(), alpha ? alpha[0] : 1.0, beta ? beta[0] : 1.0, d_ab, which, which_b, lds_a);
    HIPCHK(hipGetLastError());
    z->bound = zb;
    std::fill(z->ot.begin(), z->ot.end(), 0);
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_STREAM_H
