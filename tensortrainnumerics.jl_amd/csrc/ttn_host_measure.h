// ttn_host_measure.h — host API: site-resolved measurements.
#ifndef TTN_HOST_MEASURE_H
#define TTN_HOST_MEASURE_H
#include "ttn_host_core.h"
#include "ttn_dot_kernels.h"
#include "ttn_grad_kernels.h"
#include "ttn_measure_kernels.h"

namespace {
std::vector<double> g_measure_host;     // ttn_site_expect / ttn_correlation: the host copy of the site offsets and the operator tables, kept likewise
hipEvent_t g_measure_ev = nullptr;
DevBuf g_measure_tab;      // [d] site offsets, then the operator tables of the last ttn_site_expect / ttn_correlation
}  // namespace

extern "C" {
// ---- site-resolved measurements (include/ttn_measure.h, csrc/ttn_measure_kernels.h) ------------------------------------
static_assert(MEASURE_MAX_OPS == TTN_MEASURE_MAX_OPS, "ttn_measure.h and ttn_measure_kernels.h disagree");
// What one train needs in g_scratch (doubles), checked before anything is launched: both chains of k_grad_chain, the states V^O_k of
// `ntab` tables, and — only when a site can lie outside the on-chip class — the general route's workspace of every workgroup.
struct MeasurePlan {
    long long W = 1, tsz = 1, S = 0, wgs = 0, per_train = 0;
    bool gen = false;
};
static int measure_plan(const char* who, const ttn_tt_s* x, int ntab, int npass, MeasurePlan& M) {
    F64_ONLY(who, {x});
    const int d = x->d;
    const std::string w(who);
    if (d > MEASURE_MAX_D) return fail(TTN_ERR_UNSUPPORTED, (w + ": chains longer than 480 sites are not supported").c_str());
    if (x->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + ": a train of 2^31 doubles or more").c_str());
    long long rmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) rmax = std::max<long long>(rmax, x->bound[m]);
    for (int k = 0; k < d; ++k) {
        nmax = std::max<long long>(nmax, x->dims[k]);
        M.S += x->dims[k] * x->dims[k];
        M.gen = M.gen || x->dims[k] != 2;
    }
    M.gen = M.gen || rmax > DOT_RMAX;
    const char* big = ": ranks too large (the workspace of one train reaches 2^31 doubles)";
    if (rmax >= (1LL << 16) || nmax >= (1LL << 31) || nmax * rmax * rmax >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    M.W = (rmax * rmax + 1) & ~1LL;
    M.tsz = (nmax * rmax * rmax + 1) & ~1LL;
    M.wgs = M.gen ? std::max<long long>((long long)ntab * d, (long long)npass * (d - 1)) : 0;
    M.per_train = 2 * (d + 1) * M.W + 2 * M.tsz + (long long)ntab * d * M.W + M.wgs * (2 * M.tsz + 2 * M.W);
    if (M.per_train >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    return TTN_OK;
}

// The three phases for `ntab` host tables of M.S doubles each; d_out is device memory.  Tables t < nemit write their profile to
// d_out[b ob + t ot + k ok]; npass passes of walks (tables o1 / o2 per pass) fill d_out[b d d + ...] off the diagonal.
static int measure_run(ttn_tt_t x, const MeasurePlan& M, int ntab, const double* const* tabs, int nemit, long long ob, long long ot, long long ok, int npass,
                       const int* o1, const int* o2, bool mirror, int64_t normalize, double* d_out) {
    const int d = x->d, batch = x->batch;
    // the offsets and the tables travel from a host copy that stays untouched until the upload has completed
    if (!g_measure_ev) HIPCHK(hipEventCreateWithFlags(&g_measure_ev, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(g_measure_ev));
    g_measure_host.assign((size_t)d + (size_t)ntab * M.S, 0.0);
    {
        long long off = 0;
        for (int k = 0; k < d; ++k) { memcpy(&g_measure_host[k], &off, sizeof(off)); off += x->dims[k] * x->dims[k]; }
        for (int t = 0; t < ntab; ++t) memcpy(&g_measure_host[(size_t)d + (size_t)t * M.S], tabs[t], sizeof(double) * (size_t)M.S);
    }
    const long long chunk = std::max<long long>(1, std::min<long long>(std::min<long long>(batch, 65535),
                                                                       TTN_MEASURE_CHUNK_BYTES / (long long)(sizeof(double) * M.per_train)));
    int rc;
    if ((rc = scratch_take(sizeof(double) * (size_t)M.per_train * (size_t)chunk))) return rc;
    if ((rc = g_measure_tab.ensure(sizeof(double) * g_measure_host.size()))) return rc;
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    HIPCHK(hipMemcpyAsync(g_measure_tab.p, g_measure_host.data(), sizeof(double) * g_measure_host.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipEventRecord(g_measure_ev, g_stream));
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, batch - b0);
        TTDev xd = x->dev();
        xd.data += b0 * x->stride; xd.rks += b0 * (d + 1); xd.batch = nb;
        GradChainArgs C_;
        C_.a = xd; C_.b = xd;
        C_.env = g_scratch.as<double>();
        C_.tbuf = C_.env + (size_t)2 * (d + 1) * M.W * nb;
        C_.W = M.W; C_.tsz = M.tsz;
        C_.out = nullptr;
        hipLaunchKernelGGL(k_grad_chain, dim3(nb, 2), dim3(TTN_WG), DOT_LDS_BYTES(d), g_stream, C_);
        HIPCHK(hipGetLastError());
        MeasureArgs P;
        memset(&P, 0, sizeof(P));
        P.x = xd;
        P.env = C_.env; P.W = M.W;
        P.toff = g_measure_tab.as<long long>();
        P.tabs = g_measure_tab.as<double>() + d;
        P.S = M.S; P.ntab = ntab;
        P.V = C_.tbuf + (size_t)2 * M.tsz * nb;
        P.work = P.V + (size_t)ntab * d * M.W * nb;
        P.csz = M.tsz; P.tsz = M.tsz; P.wstride = 2 * M.tsz + 2 * M.W;
        P.out = d_out + b0 * ob;
        P.ob = ob; P.ot = ot; P.ok = ok; P.nemit = nemit;
        P.normalize = normalize ? 1 : 0;
        for (int p = 0; p < npass; ++p) { P.o1[p] = o1[p]; P.o2[p] = o2[p]; }
        P.mirror = mirror ? 1 : 0;
        hipLaunchKernelGGL(k_measure_open, dim3(d * ntab, nb), dim3(TTN_WG), MEASURE_LDS_BYTES(d), g_stream, P);
        HIPCHK(hipGetLastError());
        if (npass > 0 && d > 1) {
            hipLaunchKernelGGL(k_measure_walk, dim3(d - 1, nb, npass), dim3(TTN_WG), MEASURE_LDS_BYTES(d), g_stream, P);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    return TTN_OK;
}

static int site_expect_launch(const char* who, ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out) {
    if (nops < 1 || nops > TTN_MEASURE_MAX_OPS) return fail(TTN_ERR_ARG, (std::string(who) + ": nops must be in 1:16").c_str());
    MeasurePlan M;
    int rc;
    if ((rc = measure_plan(who, x, (int)nops, 0, M))) return rc;
    std::vector<const double*> tabs((size_t)nops);
    for (int64_t t = 0; t < nops; ++t) tabs[t] = ops + t * M.S;
    return measure_run(x, M, (int)nops, tabs.data(), (int)nops, (long long)x->d * nops, x->d, 1, 0, nullptr, nullptr, false, normalize, d_out);
}

int ttn_site_expect_dev(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !ops || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    return site_expect_launch("ttn_site_expect_dev", x, nops, ops, normalize, d_out);
}

int ttn_site_expect(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !ops || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (nops < 1 || nops > TTN_MEASURE_MAX_OPS) return fail(TTN_ERR_ARG, "ttn_site_expect: nops must be in 1:16");
    const size_t bytes = sizeof(double) * (size_t)x->d * (size_t)nops * (size_t)x->batch;
    int rc;
    { MeasurePlan M; if ((rc = measure_plan("ttn_site_expect", x, (int)nops, 0, M))) return rc; }      // every check before the first allocation
    if ((rc = g_dout.ensure(bytes))) return rc;
    if ((rc = site_expect_launch("ttn_site_expect", x, nops, ops, normalize, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, bytes, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// Tables of a correlation: 0 = P_k Q_k (the diagonal, built here), 1 = P, 2 = Q (absent when Q equals P bitwise).
static int correlation_launch(const char* who, ttn_tt_t x, const double* Pt, const double* Qt, int64_t normalize, double* d_out) {
    MeasurePlan M;
    int rc;
    if ((rc = measure_plan(who, x, 3, 2, M))) return rc;
    const int d = x->d;
    const bool same = Pt == Qt || memcmp(Pt, Qt, sizeof(double) * (size_t)M.S) == 0;
    if (same) { M = MeasurePlan(); if ((rc = measure_plan(who, x, 2, 1, M))) return rc; }
    std::vector<double> PQ((size_t)M.S);
    {
        size_t off = 0;
        for (int k = 0; k < d; ++k) {
            const int n = (int)x->dims[k];
            for (int c = 0; c < n; ++c)
                for (int r = 0; r < n; ++r) {
                    double acc = 0.0;
                    for (int w = 0; w < n; ++w) acc += Pt[off + r + (size_t)n * w] * Qt[off + w + (size_t)n * c];
                    PQ[off + r + (size_t)n * c] = acc;
                }
            off += (size_t)n * n;
        }
    }
    const double* tabs[3] = {PQ.data(), Pt, Qt};
    const int o1[2] = {same ? 1 : 2, 1}, o2[2] = {1, 2};              // pass 0: (O1, O2) = (Q, P), the upper triangle; pass 1: (P, Q), the lower
    return measure_run(x, M, same ? 2 : 3, tabs, 1, (long long)d * d, 0, d + 1, same ? 1 : 2, o1, o2, same, normalize, d_out);
}

int ttn_correlation_dev(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !P || !Q || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    return correlation_launch("ttn_correlation_dev", x, P, Q, normalize, d_out);
}

int ttn_correlation(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !P || !Q || !out) return fail(TTN_ERR_ARG, "null pointer");
    const size_t bytes = sizeof(double) * (size_t)x->d * (size_t)x->d * (size_t)x->batch;
    int rc;
    { MeasurePlan M; if ((rc = measure_plan("ttn_correlation", x, 3, 2, M))) return rc; }
    if ((rc = g_dout.ensure(bytes))) return rc;
    if ((rc = correlation_launch("ttn_correlation", x, P, Q, normalize, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, bytes, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_MEASURE_H
