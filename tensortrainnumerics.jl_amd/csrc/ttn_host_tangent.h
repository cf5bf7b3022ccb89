// ttn_host_tangent.h — host API: the fixed-rank TT manifold (include/ttn_tangent.h): tangent projection and the train alpha x + beta xi.
// Uses g_grad_coef and stream_grid of ttn_host_stream.h and stream_fibres_too_many of ttn_host_handles.h.
#ifndef TTN_HOST_TANGENT_H
#define TTN_HOST_TANGENT_H
#include "ttn_host_core.h"
#include "ttn_host_handles.h"
#include "ttn_host_stream.h"
#include "ttn_tangent_kernels.h"

extern "C" {
// ---- the fixed-rank manifold (include/ttn_tangent.h, csrc/ttn_tangent_kernels.h) -------------------------------------
// What both calls check alike before anything is launched: Float64 handles of equal dims and batch, trains below 2^31 doubles.
static int tangent_common(const char* who, std::initializer_list<const ttn_tt_s*> tts) {
    const std::string w(who);
    const ttn_tt_s* first = *tts.begin();
    for (const ttn_tt_s* h : tts) {
        if (!same_dims(first->dims, h->dims)) return fail(TTN_ERR_DIMS, (w + ": Incompatible dimensions").c_str());
        if (first->batch != h->batch) return fail(TTN_ERR_DIMS, (w + ": batch sizes differ").c_str());
    }
    if (any_c64(tts)) return refuse_c64(who);
    for (const ttn_tt_s* h : tts)
        if (h->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + ": a train of 2^31 doubles or more").c_str());
    return TTN_OK;
}

int ttn_tangent_project(ttn_tt_t U, ttn_tt_t V, ttn_tt_t z, ttn_tt_t xi, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!U || !V || !z || !xi) return fail(TTN_ERR_ARG, "ttn_tangent_project: null handle");
    if (xi == U || xi == V || xi == z) return fail(TTN_ERR_ARG, "ttn_tangent_project: the destination must not alias an operand");
    int rc = tangent_common("ttn_tangent_project", {U, V, z, xi});
    if (rc) return rc;
    const int d = U->d, batch = U->batch;
    if (d > DOT_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_project: chains longer than 480 sites are not supported");
    for (int m = 0; m <= d; ++m)
        if (xi->cap[m] < U->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_tangent_project: destination capacity too small");
    // workspace per train: both chains with every state, 2 (d + 1) W doubles, W = max_m r_m rz_m, and one GEMM intermediate per chain.
    // A train passes the device's rank check only when V's ranks are U's, so U's bounds hold for both bras.
    long long W = 1, rmax = 1, rzmax = 1, nmax = 1, tiles = 1;
    for (int m = 0; m <= d; ++m) {
        if (U->bound[m] >= (1LL << 31) || z->bound[m] >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_project: ranks too large");
        W = std::max<long long>(W, U->bound[m] * z->bound[m]);
        rmax = std::max<long long>(rmax, U->bound[m]); rzmax = std::max<long long>(rzmax, z->bound[m]);
    }
    for (int k = 0; k < d; ++k) {
        nmax = std::max<long long>(nmax, U->dims[k]);
        tiles = std::max<long long>(tiles, ((U->bound[k] + 15) / 16) * ((U->bound[k + 1] + 63) / 64));
    }
    W = (W + 1) & ~1LL;
    if (rmax * rzmax >= (1LL << 31) / nmax) return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_project: ranks too large (the workspace of one train reaches 2^31 doubles)");
    const long long tsz = (nmax * rmax * rzmax + 1) & ~1LL;
    const long long per_train = 2 * (d + 1) * W + 2 * tsz;
    if (per_train >= (1LL << 31) || tiles >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_project: ranks too large (the workspace of one train reaches 2^31 doubles)");
    // trains per chunk: what keeps the workspace within TTN_TANGENT_CHUNK_BYTES (one train at least), and the grid's 65535
    const long long budget = TTN_TANGENT_CHUNK_BYTES / (long long)sizeof(double);
    const long long chunk = std::max<long long>(1, std::min<long long>(std::min<long long>(batch, 65535), budget / per_train));
    if ((rc = scratch_take(sizeof(double) * (size_t)per_train * (size_t)chunk))) return rc;
    if (out && (rc = g_dout.ensure(sizeof(double) * batch))) return rc;
    // xi becomes a tangent at x: U's ranks (copied on the device), its host-side bounds, gauge flags 0
    hipLaunchKernelGGL(k_ranks_copy, dim3(batch), dim3(64), 0, g_stream, xi->dev(), U->dev());
    HIPCHK(hipGetLastError());
    xi->bound = U->bound;
    std::fill(xi->ot.begin(), xi->ot.end(), 0);
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, batch - b0);
        auto part = [&](ttn_tt_t h) {
            TTDev t = h->dev();
            t.data += b0 * h->stride; t.rks += b0 * (d + 1); t.batch = nb;
            return t;
        };
        TangentChainArgs C_;
        C_.u = part(U); C_.v = part(V); C_.z = part(z);
        C_.env = g_scratch.as<double>();
        C_.tbuf = C_.env + (size_t)2 * (d + 1) * W * nb;
        C_.W = W; C_.tsz = tsz;
        C_.out = out ? g_dout.as<double>() + b0 : nullptr;
        hipLaunchKernelGGL(k_tangent_chain, dim3(nb, 2), dim3(TTN_WG), DOT_LDS_BYTES(d), g_stream, C_);
        HIPCHK(hipGetLastError());
        TangentSandArgs S_;
        S_.u = C_.u; S_.v = C_.v; S_.z = C_.z; S_.xi = part(xi);
        S_.env = C_.env; S_.W = W;
        S_.status = xi->d_status + b0;
        hipLaunchKernelGGL(k_tangent_sandwich, dim3((unsigned)tiles, d, nb), dim3(GRAD_SW_TB), 0, g_stream, S_);
        HIPCHK(hipGetLastError());
    }
    if (out) {
        HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return TTN_OK;
}

int ttn_tangent_to_tt(ttn_tt_t U, ttn_tt_t V, ttn_tt_t xi, const double* alpha, const double* beta, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!U || !V || !xi || !y) return fail(TTN_ERR_ARG, "ttn_tangent_to_tt: null handle");
    if (y == U || y == V || y == xi) return fail(TTN_ERR_ARG, "ttn_tangent_to_tt: the destination must not alias an operand");
    int rc = tangent_common("ttn_tangent_to_tt", {U, V, xi, y});
    if (rc) return rc;
    const int d = U->d, batch = U->batch;
    for (int m = 1; m < d; ++m)
        if (y->cap[m] < 2 * U->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_tangent_to_tt: destination capacity below twice the ranks of U");
    if (batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_to_tt: more than 65535 trains");
    long long items = 1;
    for (int k = 0; k < d; ++k) {
        const long long zl = k == 0 ? 1 : 2 * U->bound[k], zr = k == d - 1 ? 1 : 2 * U->bound[k + 1];
        if (U->bound[k] >= (1LL << 30) || U->bound[k + 1] >= (1LL << 30) || stream_fibres_too_many(zl * zr))
            return fail(TTN_ERR_UNSUPPORTED, "ttn_tangent_to_tt: 2^31 or more fibres in one output core (32-bit element indices)");
        items = std::max<long long>(items, U->dims[k] == 2 ? zl * ((zr + TTN_TAN_K - 1) / TTN_TAN_K) : zl * zr);
    }
    // `batch` host doubles each into the halves of g_grad_coef (null: no copy, the kernel takes 1).  Synchronises: caller memory.
    const double* d_alpha = nullptr; const double* d_beta = nullptr;
    if (alpha || beta) {
        if ((rc = g_grad_coef.ensure(sizeof(double) * 2 * (size_t)batch))) return rc;
        double* p = g_grad_coef.as<double>();
        if (alpha) { HIPCHK(hipMemcpyAsync(p, alpha, sizeof(double) * batch, hipMemcpyHostToDevice, g_stream)); d_alpha = p; }
        if (beta) { HIPCHK(hipMemcpyAsync(p + batch, beta, sizeof(double) * batch, hipMemcpyHostToDevice, g_stream)); d_beta = p + batch; }
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    TangentAsmArgs A_;
    A_.u = U->dev(); A_.v = V->dev(); A_.xi = xi->dev(); A_.y = y->dev();
    A_.alpha = d_alpha; A_.beta = d_beta;
    A_.status = y->d_status;
    hipLaunchKernelGGL(k_tangent_assemble, stream_grid(items, d, batch), dim3(TTN_STREAM_TB), 0, g_stream, A_);
    HIPCHK(hipGetLastError());
    for (int m = 0; m <= d; ++m) y->bound[m] = (m == 0 || m == d) ? 1 : 2 * U->bound[m];
    std::fill(y->ot.begin(), y->ot.end(), 0);
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_TANGENT_H
