// ttn_host_rect.h — host API: rectangular TT operators: the ttn_rtto handle and ttn_apply_rect.
#ifndef TTN_HOST_RECT_H
#define TTN_HOST_RECT_H
#include "ttn_host_core.h"
#include "ttn_host_handles.h"
#include "ttn_host_stream.h"
#include "ttn_rect_kernels.h"

extern "C" {
// ---- rectangular operators (csrc/ttn_rect_kernels.h) ------------------------------------------------------------------------------
int ttn_rtto_create(int64_t M, const int64_t* out_dims, const int64_t* in_dims, const int64_t* rks, const double* const* cores, ttn_rtto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!out_dims || !in_dims || !rks || !cores || !out || M < 1 || M > TTN_MAX_D) return fail(TTN_ERR_ARG, "ttn_rtto_create: bad argument");
    for (int64_t k = 0; k < M; ++k) {
        if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_rtto_create: null core");
        if (out_dims[k] < 1 || in_dims[k] < 1) return fail(TTN_ERR_ARG, "ttn_rtto_create: dims must be >= 1");
    }
    for (int64_t k = 0; k <= M; ++k) if (rks[k] < 1) return fail(TTN_ERR_ARG, "ttn_rtto_create: ranks must be >= 1");
    OwnedRTTO own;
    ttn_rtto_s* h = own.h = new ttn_rtto_s();
    h->d = (int)M;
    h->odims.assign(out_dims, out_dims + M);
    h->idims.assign(in_dims, in_dims + M);
    h->rks.assign(rks, rks + M + 1);
    h->off.resize(M + 1);
    long long o = 0;
    for (int64_t k = 0; k < M; ++k) {
        h->off[k] = o;
        if (in_dims[k] == 1) h->singles.push_back((int)k);
        const long long sz = (long long)out_dims[k] * in_dims[k] * rks[k] * rks[k + 1];
        o += (sz + 1) & ~1LL;      // keep every slot 16-byte aligned
    }
    h->off[M] = o;
    std::vector<int> idims(2 * M);
    for (int64_t k = 0; k < M; ++k) { idims[k] = (int)out_dims[k]; idims[M + k] = (int)in_dims[k]; }
    std::vector<long long> r64(rks, rks + M + 1);
    std::vector<double> flat((size_t)o, 0.0);                           // the cores at their slots, the rounding gaps zero
    for (int64_t k = 0; k < M; ++k) std::memcpy(flat.data() + h->off[k], cores[k], sizeof(double) * (size_t)out_dims[k] * in_dims[k] * rks[k] * rks[k + 1]);
    hipError_t e;
    if ((e = hipMalloc((void**)&h->d_data, sizeof(double) * (size_t)o)) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_off, sizeof(long long) * (M + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_rks, sizeof(long long) * (M + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_dims, sizeof(int) * 2 * M)) != hipSuccess)
        return hipfail(e, "hipMalloc(ttn_rtto)");
    HIPCHK(hipMemcpyAsync(h->d_data, flat.data(), sizeof(double) * (size_t)o, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_off, h->off.data(), sizeof(long long) * (M + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_rks, r64.data(), sizeof(long long) * (M + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_dims, idims.data(), sizeof(int) * 2 * M, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));          // the tables and `flat` are locals, `cores` is caller memory
    *out = own.release();
    return TTN_OK;
}

int ttn_rtto_free(ttn_rtto_t h) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!h) return TTN_OK;
    if (g_init) hipStreamSynchronize(g_stream);
    if (h->d_data) hipFree(h->d_data);
    if (h->d_off) hipFree(h->d_off);
    if (h->d_rks) hipFree(h->d_rks);
    if (h->d_dims) hipFree(h->d_dims);
    delete h;
    return TTN_OK;
}

int ttn_rtto_ranks(ttn_rtto_t h, int64_t* M, int64_t* out_dims, int64_t* in_dims, int64_t* rks) {
    if (!h) return fail(TTN_ERR_ARG, "null handle");
    if (M) *M = h->d;
    for (int k = 0; k < h->d; ++k) { if (out_dims) out_dims[k] = h->odims[k]; if (in_dims) in_dims[k] = h->idims[k]; }
    if (rks) for (int m = 0; m <= h->d; ++m) rks[m] = h->rks[m];
    return TTN_OK;
}

// y = A * x for a rectangular A (src/tt_operations.jl:116-148).  Every check runs before y is touched.
int ttn_apply_rect(ttn_rtto_t A, ttn_tt_t x, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !x || !y) return fail(TTN_ERR_ARG, "null handle");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_apply_rect: output must not alias the input");
    F64_ONLY("ttn_apply_rect", {x, y});
    const int M = A->d, N = x->d;
    if (M != N + 1) return fail(TTN_ERR_DIMS, "Rectangular TToperator must have one additional output site");
    if (A->singles.size() != 1) return fail(TTN_ERR_DIMS, "Rectangular TToperator must have exactly one singleton input site");
    const int s = A->singles[0];
    for (int k = 0; k < N; ++k) if (A->idims[k < s ? k : k + 1] != x->dims[k]) return fail(TTN_ERR_DIMS, "Incompatible input dimensions");
    if (x->bound[N] != 1) return fail(TTN_ERR_DIMS, "Input TTvector must have a closed right boundary rank");
    if (y->d != M || !same_dims(A->odims, y->dims)) return fail(TTN_ERR_DIMS, "ttn_apply_rect: the destination's dimensions are not the operator's output dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    std::vector<int64_t> yb(M + 1);
    for (int m = 0; m <= M; ++m) yb[m] = A->rks[m] * x->bound[m > s ? m - 1 : m];
    for (int m = 0; m <= M; ++m) if (y->cap[m] < yb[m]) return fail(TTN_ERR_CAPACITY, "ttn_apply_rect: destination capacity too small");
    for (int k = 0; k < M; ++k)
        if (stream_fibres_too_many((long long)y->cap[k] * y->cap[k + 1])) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply_rect: 2^31 or more fibres in one output core (32-bit element indices)");
    // LDS: the largest operator core that takes the n_out = 2 mapping and fits TTN_APPLY_LDS_DOUBLES; grid: the most items of any site
    long long lds_a = 0, items = 1;
    for (int k = 0; k < M; ++k) {
        const long long asz = (long long)A->odims[k] * A->idims[k] * A->rks[k] * A->rks[k + 1];
        const bool fast = A->odims[k] == 2 && A->idims[k] == (k == s ? 1 : 2) && asz <= TTN_APPLY_LDS_DOUBLES;
        if (fast) lds_a = std::max<long long>(lds_a, asz);
        items = std::max<long long>(items, fast ? yb[k] * ((yb[k + 1] + TTN_RECT_K - 1) / TTN_RECT_K) : yb[k] * yb[k + 1]);
    }
    hipLaunchKernelGGL(k_ranks_mul_rect, dim3(x->batch), dim3(64), 0, g_stream, y->dev(), A->dev(), x->dev());
    HIPCHK(hipGetLastError());
    y->bound = yb;
    std::fill(y->ot.begin(), y->ot.end(), 0);
    hipLaunchKernelGGL(k_apply_rect, stream_grid(items, M, x->batch), dim3(TTN_STREAM_TB), sizeof(double) * (size_t)((lds_a + 1) & ~1LL), g_stream,
                       A->dev(), x->dev(), y->dev(), (int)lds_a);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_RECT_H
