// ttn_host_handles.h — host API: the train and operator handles: create, free, upload, download, ranks, copy, element type.
// tto_alloc is the one place that lays out an operator handle (the operator algebra and the operator batches allocate their results with
// it); stream_fibres_too_many, the 32-bit fibre bound of the streaming kernels, stands here because tto_alloc is the lowest of its users.
#ifndef TTN_HOST_HANDLES_H
#define TTN_HOST_HANDLES_H
#include "ttn_host_core.h"
#include "ttn_stream_kernels.h"

extern "C" {
// r_and_d_to_rks with Julia's wrapping Int64 products (src/tt_tools.jl:407-425)
static int64_t wrap_prod(const int64_t* v, int64_t lo, int64_t hi) {  // product of v[lo..hi)
    uint64_t p = 1;
    for (int64_t i = lo; i < hi; ++i) p *= (uint64_t)v[i];
    return (int64_t)p;
}
int ttn_r_and_d_to_rks(int64_t d, const int64_t* dims, int64_t n_rks, const int64_t* rks, int64_t rmax, int64_t* out) {
    if (!dims || !rks || !out || d < 0 || n_rks < 0) return fail(TTN_ERR_ARG, "bad argument");
    for (int64_t i = 0; i < n_rks; ++i) out[i] = 1;
    for (int64_t i = 0; i < d && i < n_rks; ++i) {
        const int64_t q = wrap_prod(dims, i, d), p = wrap_prod(dims, 0, i);
        int64_t v = rks[i];
        if (q > 0) {
            if (p > 0) v = std::min(std::min(v, p), std::min(q, rmax));
            else v = std::min(v, std::min(q, rmax));
        } else {
            if (p > 0) v = std::min(v, std::min(p, rmax));
            else v = std::min(v, rmax);
        }
        out[i] = v;
    }
    return TTN_OK;
}

// ---- ttn_tt ---------------------------------------------------------------------------------------
static int tt_create_impl(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out, int el);
int ttn_tt_create(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out) { return tt_create_impl(d, dims, cap_rks, batch, out, 1); }
int ttn_tt_create_c64(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out) { return tt_create_impl(d, dims, cap_rks, batch, out, 2); }
int ttn_tt_dtype(ttn_tt_t h, int* cplx) {
    if (!h || !cplx) return fail(TTN_ERR_ARG, "null pointer");
    *cplx = h->el == 2 ? 1 : 0;
    return TTN_OK;
}
int ttn_tto_dtype(ttn_tto_t h, int* cplx) {
    if (!h || !cplx) return fail(TTN_ERR_ARG, "null pointer");
    *cplx = h->el == 2 ? 1 : 0;
    return TTN_OK;
}
static int tt_create_impl(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out, int el) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!dims || !cap_rks || !out || d < 1 || batch < 1) return fail(TTN_ERR_ARG, "ttn_tt_create: bad argument");
    for (int64_t k = 0; k < d; ++k) if (dims[k] < 1) return fail(TTN_ERR_ARG, "ttn_tt_create: dims must be >= 1");
    for (int64_t k = 0; k <= d; ++k) if (cap_rks[k] < 1) return fail(TTN_ERR_ARG, "ttn_tt_create: ranks must be >= 1");
    OwnedTT own;
    ttn_tt_s* h = own.h = new ttn_tt_s();
    h->d = (int)d; h->batch = (int)batch; h->el = el;
    h->dims.assign(dims, dims + d);
    h->cap.assign(cap_rks, cap_rks + d + 1);
    h->bound.assign(d + 1, 1);          // every train starts as the rank-1 zero train
    h->off.resize(d + 1);
    long long o = 0;
    for (int64_t k = 0; k < d; ++k) {
        h->off[k] = o;
        long long sz = (long long)el * dims[k] * cap_rks[k] * cap_rks[k + 1];
        sz = (sz + 1) & ~1LL;      // keep every slot 16-byte aligned
        o += sz;
    }
    h->off[d] = o;
    h->stride = o;
    h->ot.assign((size_t)batch * d, 0);
    std::vector<int> idims(d);
    for (int64_t k = 0; k < d; ++k) idims[k] = (int)(el * dims[k]);
    std::vector<long long> cap64(cap_rks, cap_rks + d + 1);
    std::vector<long long> rk0((size_t)batch * (d + 1));
    for (int64_t b = 0; b < batch; ++b) for (int64_t m = 0; m <= d; ++m) rk0[b * (d + 1) + m] = 1;
    hipError_t e;
    if ((e = hipMalloc((void**)&h->d_data, sizeof(double) * (size_t)o * batch)) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_off, sizeof(long long) * (d + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_cap, sizeof(long long) * (d + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_rks, sizeof(long long) * (size_t)batch * (d + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_dims, sizeof(int) * d)) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_status, sizeof(int) * 2 * (size_t)batch)) != hipSuccess)
        return hipfail(e, "hipMalloc(ttn_tt)");
    HIPCHK(hipMemcpyAsync(h->d_off, h->off.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_cap, cap64.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_rks, rk0.data(), sizeof(long long) * rk0.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_dims, idims.data(), sizeof(int) * d, hipMemcpyHostToDevice, g_stream));
    { const int rc = fresh_fill(h->d_data, sizeof(double) * (size_t)o * batch, true); if (rc) return rc; }
    if (g_poison)                                      // the live block of the rank-1 zero train: el * n_k doubles at the start of every slot
        for (int64_t k = 0; k < d; ++k)
            HIPCHK(hipMemset2DAsync(h->d_data + h->off[k], sizeof(double) * (size_t)o, 0, sizeof(double) * (size_t)el * dims[k], (size_t)batch, g_stream));
    HIPCHK(hipMemsetAsync(h->d_status, 0, sizeof(int) * 2 * (size_t)batch, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    g_live.insert(h);
    *out = own.release();
    return TTN_OK;
}

int ttn_tt_free(ttn_tt_t h) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!h) return TTN_OK;
    const bool was_live = g_live.erase(h) > 0;
    if (g_init && was_live && h->d_status) {
        // a failure recorded on this handle that nobody has queried survives the handle (ttn_status_all)
        hipLaunchKernelGGL(k_fold_status, dim3(1), dim3(64), 0, g_stream, (const int*)h->d_status, h->batch, g_pending_status.as<unsigned>());
    }
    if (g_init) hipStreamSynchronize(g_stream);
    if (h->d_data) hipFree(h->d_data);
    if (h->d_off) hipFree(h->d_off);
    if (h->d_cap) hipFree(h->d_cap);
    if (h->d_rks) hipFree(h->d_rks);
    if (h->d_dims) hipFree(h->d_dims);
    if (h->d_sv) hipFree(h->d_sv);
    if (h->d_status) hipFree(h->d_status);
    delete h;
    return TTN_OK;
}

int ttn_tt_batch(ttn_tt_t h, int64_t* batch) {
    if (!h || !batch) return fail(TTN_ERR_ARG, "null pointer");
    *batch = h->batch;
    return TTN_OK;
}

int ttn_tt_upload(ttn_tt_t h, int64_t b, const double* const* cores, const int64_t* rks, const int64_t* ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || !cores || !rks || b < 0 || b >= h->batch) return fail(TTN_ERR_ARG, "ttn_tt_upload: bad argument");
    const int d = h->d;
    for (int m = 0; m <= d; ++m) {
        if (rks[m] < 1) return fail(TTN_ERR_ARG, "ttn_tt_upload: ranks must be >= 1");
        if (rks[m] > h->cap[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_upload: rank exceeds the handle's capacity");
    }
    std::vector<long long> r64(rks, rks + d + 1);
    HIPCHK(hipMemcpyAsync(h->d_rks + (size_t)b * (d + 1), r64.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    for (int k = 0; k < d; ++k) {
        if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_tt_upload: null core");
        const size_t sz = (size_t)h->el * h->dims[k] * rks[k] * rks[k + 1];
        HIPCHK(hipMemcpyAsync(h->d_data + (size_t)b * h->stride + h->off[k], cores[k], sizeof(double) * sz, hipMemcpyHostToDevice, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));   // host buffers may be released by the caller
    for (int k = 0; k < d; ++k) h->ot[(size_t)b * d + k] = ot ? ot[k] : 0;
    // host-side upper bound on the current ranks of any train of the batch
    for (int m = 0; m <= d; ++m) h->bound[m] = (h->batch == 1) ? rks[m] : std::max<int64_t>(h->bound[m], rks[m]);
    return TTN_OK;
}

int ttn_tt_replicate(ttn_tt_t h, int64_t src_b) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || src_b < 0 || src_b >= h->batch) return fail(TTN_ERR_ARG, "ttn_tt_replicate: bad argument");
    if (h->batch > 1) {
        dim3 grid((unsigned)std::min<long long>((h->stride + TTN_STREAM_TB - 1) / TTN_STREAM_TB, 1024), (unsigned)h->batch);
        hipLaunchKernelGGL(k_replicate, grid, dim3(TTN_STREAM_TB), 0, g_stream, h->dev(), (int)src_b);
        HIPCHK(hipGetLastError());
    }
    for (int b = 0; b < h->batch; ++b)
        for (int k = 0; k < h->d; ++k) h->ot[(size_t)b * h->d + k] = h->ot[(size_t)src_b * h->d + k];
    return TTN_OK;
}

int ttn_tt_ranks(ttn_tt_t h, int64_t b, int64_t* rks, int64_t* ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || b < 0 || b >= h->batch) return fail(TTN_ERR_ARG, "ttn_tt_ranks: bad argument");
    const int d = h->d;
    if (rks) {
        std::vector<long long> r64(d + 1);
        HIPCHK(hipMemcpyAsync(r64.data(), h->d_rks + (size_t)b * (d + 1), sizeof(long long) * (d + 1), hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        for (int m = 0; m <= d; ++m) rks[m] = r64[m];
    }
    if (ot) for (int k = 0; k < d; ++k) ot[k] = h->ot[(size_t)b * d + k];
    return TTN_OK;
}

int ttn_tt_max_ranks(ttn_tt_t h, int64_t* bound) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h) return fail(TTN_ERR_ARG, "null handle");
    const int d = h->d;
    std::vector<long long> r64((size_t)h->batch * (d + 1));
    HIPCHK(hipMemcpyAsync(r64.data(), h->d_rks, sizeof(long long) * r64.size(), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int m = 0; m <= d; ++m) {
        long long mx = 1;
        for (int b = 0; b < h->batch; ++b) mx = std::max(mx, r64[(size_t)b * (d + 1) + m]);
        h->bound[m] = mx;
        if (bound) bound[m] = mx;
    }
    return TTN_OK;
}

int ttn_tt_download(ttn_tt_t h, int64_t b, double* const* cores) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || !cores || b < 0 || b >= h->batch) return fail(TTN_ERR_ARG, "ttn_tt_download: bad argument");
    const int d = h->d;
    std::vector<long long> r64(d + 1);
    HIPCHK(hipMemcpyAsync(r64.data(), h->d_rks + (size_t)b * (d + 1), sizeof(long long) * (d + 1), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int k = 0; k < d; ++k) {
        if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_tt_download: null core");
        const size_t sz = (size_t)h->el * h->dims[k] * r64[k] * r64[k + 1];
        HIPCHK(hipMemcpyAsync(cores[k], h->d_data + (size_t)b * h->stride + h->off[k], sizeof(double) * sz, hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

int ttn_tt_copy(ttn_tt_t dst, ttn_tt_t src) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!dst || !src) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(dst->dims, src->dims) || dst->batch != src->batch) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (dst->el != src->el) return refuse_mixed("ttn_tt_copy");
    for (int m = 0; m <= src->d; ++m) if (dst->cap[m] < src->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_copy: destination capacity too small");
    // scale kernel with a = 1 on core -1 is a plain per-core copy that honours the two slot layouts
    const int d = src->d;
    long long maxsz = 0;
    for (int k = 0; k < d; ++k) maxsz = std::max<long long>(maxsz, (long long)src->el * src->dims[k] * src->bound[k] * src->bound[k + 1]);
    hipLaunchKernelGGL(k_ranks_copy, dim3(src->batch), dim3(64), 0, g_stream, dst->dev(), src->dev());
    dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((maxsz + TTN_STREAM_TB - 1) / TTN_STREAM_TB, 2048)), (unsigned)d, (unsigned)src->batch);
    hipLaunchKernelGGL(k_scale, grid, dim3(TTN_STREAM_TB), 0, g_stream, src->dev(), dst->dev(), 1.0, -1, 0, (const int*)nullptr);
    HIPCHK(hipGetLastError());
    dst->bound = src->bound;
    dst->ot = src->ot;
    return TTN_OK;
}

// ---- ttn_tto --------------------------------------------------------------------------------------
// k_apply / k_hadamard / k_add count the fibres (p, q) of a core with 32-bit indices (ttn_stream_kernels.h): refuse larger cores here
static bool stream_fibres_too_many(long long fibres) { return fibres >= (1LL << 31); }

// The one place that lays out and allocates an operator handle: slots, device tables and, with `cores`, their upload.  A ttn_tto is
// immutable and its ranks are host-known, so every operation of the operator algebra allocates its result here (`who`: its name) with
// the cores left uninitialised: an output core beyond the 32-bit fibre indices of the streaming kernels is refused, and a result the
// device cannot hold is TTN_ERR_CAPACITY (nothing is launched).  ttn_tto_create passes no `who` and reports the HIP error itself.
static int tto_alloc(const char* who, int el, int64_t d, const int64_t* dims, const int64_t* rks, const int64_t* ot, const double* const* cores,
                     OwnedTTO& out, int64_t batch = 1 /* operators of these dims and ranks; cores: [batch * d] */) {
    if (who)
        for (int64_t k = 0; k < d; ++k)
            if (stream_fibres_too_many((long long)rks[k] * rks[k + 1]))
                return fail(TTN_ERR_UNSUPPORTED, (std::string(who) + ": 2^31 or more fibres in one output core (32-bit element indices)").c_str());
    ttn_tto_s* h = out.h = new ttn_tto_s();
    h->d = (int)d; h->el = el; h->batch = (int)batch;
    h->dims.assign(dims, dims + d);
    h->rks.assign(rks, rks + d + 1);
    h->ot.assign(d, 0);
    if (ot) h->ot.assign(ot, ot + d);
    h->off.resize(d + 1);
    long long o = 0;
    for (int64_t k = 0; k < d; ++k) {
        h->off[k] = o;
        const long long sz = (long long)el * dims[k] * dims[k] * rks[k] * rks[k + 1];
        o += (sz + 1) & ~1LL;      // keep every slot 16-byte aligned
    }
    h->off[d] = o;
    h->stride = o;
    std::vector<int> idims(2 * d);
    for (int64_t k = 0; k < d; ++k) { idims[k] = (int)dims[k]; idims[d + k] = (int)(el * dims[k] * dims[k]); }
    std::vector<long long> r64(rks, rks + d + 1);
    hipError_t e = hipMalloc((void**)&h->d_data, sizeof(double) * (size_t)std::max<long long>(o, 1) * (size_t)batch);
    if (e != hipSuccess && who) {
        (void)hipGetLastError();
        h->d_data = nullptr;
        return fail(TTN_ERR_CAPACITY, (std::string(who) + ": the result does not fit in device memory").c_str());
    }
    if (e != hipSuccess ||
        (e = hipMalloc((void**)&h->d_off, sizeof(long long) * (d + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_rks, sizeof(long long) * (d + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&h->d_dims, sizeof(int) * 2 * d)) != hipSuccess)
        return hipfail(e, "hipMalloc(ttn_tto)");
    h->d_dims2 = h->d_dims + d;
    std::vector<double> flat;                           // the cores at their slots, the rounding gaps zero
    if (!cores) {                                       // the producing kernels write every core whole; raw unless poison mode fills it
        const int rc = fresh_fill(h->d_data, sizeof(double) * (size_t)std::max<long long>(o, 1) * (size_t)batch, false);
        if (rc) return rc;
    } else {
        double gap = 0.0;                               // (poison mode: the pattern in the gaps)
        if (g_poison) std::memcpy(&gap, &g_poison_pat, sizeof(gap));
        flat.assign((size_t)o * (size_t)batch, gap);
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t k = 0; k < d; ++k)
                std::memcpy(flat.data() + (size_t)b * (size_t)o + h->off[k], cores[b * d + k], sizeof(double) * (size_t)el * dims[k] * dims[k] * rks[k] * rks[k + 1]);
        HIPCHK(hipMemcpyAsync(h->d_data, flat.data(), sizeof(double) * flat.size(), hipMemcpyHostToDevice, g_stream));
    }
    HIPCHK(hipMemcpyAsync(h->d_off, h->off.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_rks, r64.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(h->d_dims, idims.data(), sizeof(int) * 2 * d, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));          // the tables and `flat` are locals, `cores` is caller memory
    return TTN_OK;
}

static int tto_create_impl(int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores, ttn_tto_t* out, int el) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!dims || !rks || !cores || !out || d < 1) return fail(TTN_ERR_ARG, "ttn_tto_create: bad argument");
    for (int64_t k = 0; k < d; ++k) if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_tto_create: null core");
    OwnedTTO A;
    const int rc = tto_alloc(nullptr, el, d, dims, rks, nullptr, cores, A);
    if (rc) return rc;
    *out = A.release();
    return TTN_OK;
}
int ttn_tto_create(int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores, ttn_tto_t* out) { return tto_create_impl(d, dims, rks, cores, out, 1); }
int ttn_tto_create_c64(int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores, ttn_tto_t* out) { return tto_create_impl(d, dims, rks, cores, out, 2); }

int ttn_tto_free(ttn_tto_t h) {
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

int ttn_tto_set_ot(ttn_tto_t A, const int64_t* ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!A || !ot) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_set_ot")) return rb;
    A->ot.assign(ot, ot + A->d);
    return TTN_OK;
}

int ttn_tto_ranks(ttn_tto_t A, int64_t* d, int64_t* dims, int64_t* rks, int64_t* ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!A) return fail(TTN_ERR_ARG, "null handle");
    if (d) *d = A->d;
    if (dims) for (int k = 0; k < A->d; ++k) dims[k] = A->dims[k];
    if (rks) for (int m = 0; m <= A->d; ++m) rks[m] = A->rks[m];
    if (ot) for (int k = 0; k < A->d; ++k) ot[k] = A->ot[k];
    return TTN_OK;
}

int ttn_tto_download(ttn_tto_t A, double* const* cores) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !cores) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_download")) return rb;
    for (int k = 0; k < A->d; ++k) {
        if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_tto_download: null core");
        const size_t sz = (size_t)A->el * A->dims[k] * A->dims[k] * A->rks[k] * A->rks[k + 1];
        HIPCHK(hipMemcpyAsync(cores[k], A->d_data + A->off[k], sizeof(double) * sz, hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_HANDLES_H
