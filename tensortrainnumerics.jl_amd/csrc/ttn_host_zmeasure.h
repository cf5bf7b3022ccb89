// ttn_host_zmeasure.h — host API: site-resolved measurements on ComplexF64 trains (include/ttn_zmeasure.h).
#ifndef TTN_HOST_ZMEASURE_H
#define TTN_HOST_ZMEASURE_H
#include "ttn_host_core.h"
#include "ttn_zmeasure_kernels.h"

namespace {
std::vector<double> g_zmeasure_host;    // ttn_zsite_expect / ttn_zcorrelation: the host copy of the site offsets and the operator tables
hipEvent_t g_zmeasure_ev = nullptr;     // ... which stays untouched until this event (the upload) has completed
DevBuf g_zmeasure_tab;     // [d] site offsets, then the interleaved operator tables of the last call

// the three phases of one route, on the library stream
template <bool CHIP>
static void zmeasure_phases(const ZMeasureArgs& P, int d, int nb, int ntab, int npass) {
    const size_t lds = ZM_LDS_BYTES(d);
    hipLaunchKernelGGL((k_zmeasure_chain<CHIP>), dim3(nb, 2), dim3(TTN_WG), lds, g_stream, P);
    hipLaunchKernelGGL((k_zmeasure_open<CHIP>), dim3(d * ntab, nb), dim3(TTN_WG), lds, g_stream, P);
    if (npass > 0 && d > 1) hipLaunchKernelGGL((k_zmeasure_walk<CHIP>), dim3(d - 1, nb, npass), dim3(TTN_WG), lds, g_stream, P);
}
}  // namespace

extern "C" {
// ---- site-resolved measurements on ComplexF64 trains (include/ttn_zmeasure.h, csrc/ttn_zmeasure_kernels.h) --------------
static_assert(ZMEASURE_MAX_OPS == TTN_ZMEASURE_MAX_OPS, "ttn_zmeasure.h and ttn_zmeasure_kernels.h disagree");
// What one train needs in g_scratch (doubles), checked before anything is launched — the formula of ttn_zmeasure.h.
struct ZMeasurePlan {
    long long W = 2, N = 2, S = 0, wgs = 0, per_train = 0;
    bool chip = false, gen = false;     // the on-chip kernels run (every n_k = 2) / the general ones run (a train of the batch may lie outside the class)
};
static int zmeasure_plan(const char* who, const ttn_tt_s* x, int ntab, int npass, ZMeasurePlan& M) {
    const std::string w(who);
    if (x->el != 2) return fail(TTN_ERR_UNSUPPORTED, (w + ": ComplexF64 only; a Float64 handle is measured by ttn_site_expect / ttn_correlation").c_str());
    const int d = x->d;
    if (d > ZMEASURE_MAX_D) return fail(TTN_ERR_UNSUPPORTED, (w + ": chains longer than 480 sites are not supported").c_str());
    if (x->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + ": a train of 2^31 doubles or more").c_str());
    long long rmax = 1, nmax = 1;
    M.chip = true;
    for (int m = 0; m <= d; ++m) rmax = std::max<long long>(rmax, x->bound[m]);
    for (int k = 0; k < d; ++k) {
        nmax = std::max<long long>(nmax, x->dims[k]);
        M.S += x->dims[k] * x->dims[k];
        M.chip = M.chip && x->dims[k] == 2;
    }
    // rank bounds above the limit: a ragged batch can still hold trains below it, so both routes run
    M.gen = !M.chip || rmax > ZMEASURE_RMAX;
    const char* big = ": ranks too large (the workspace of one train reaches 2^31 doubles)";
    if (rmax >= (1LL << 15) || nmax >= (1LL << 30) || 2 * nmax * rmax * rmax >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    M.W = std::max<long long>(M.chip ? ZM_STATE : 0, M.gen ? 2 * rmax * rmax : 0);
    M.N = 2 * nmax * rmax * rmax;
    M.wgs = std::max<long long>((long long)ntab * d, (long long)npass * (d - 1));
    M.per_train = 2 * (d + 1) * M.W + (long long)ntab * d * M.W + (long long)npass * (d - 1) * 2 * M.W + (M.gen ? 2 * M.N + M.wgs * 2 * M.N : 0);
    if (M.per_train >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    return TTN_OK;
}

// The three phases for `ntab` host tables of 2 M.S doubles each; d_out is device memory (interleaved).  Tables t < nemit write their
// profile to element d_out[b ob + t ot + k ok]; npass passes of walks (tables o1 / o2 per pass) fill d_out[b d d + ...] off the diagonal.
static int zmeasure_run(ttn_tt_t x, const ZMeasurePlan& M, int ntab, const double* const* tabs, int nemit, long long ob, long long ot, long long ok, int npass,
                        const int* o1, const int* o2, bool mirror, int64_t normalize, double* d_out) {
    const int d = x->d, batch = x->batch;
    if (!g_zmeasure_ev) HIPCHK(hipEventCreateWithFlags(&g_zmeasure_ev, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(g_zmeasure_ev));
    g_zmeasure_host.assign((size_t)d + (size_t)ntab * 2 * M.S, 0.0);
    {
        long long off = 0;
        for (int k = 0; k < d; ++k) { memcpy(&g_zmeasure_host[k], &off, sizeof(off)); off += x->dims[k] * x->dims[k]; }
        for (int t = 0; t < ntab; ++t) memcpy(&g_zmeasure_host[(size_t)d + (size_t)t * 2 * M.S], tabs[t], sizeof(double) * 2 * (size_t)M.S);
    }
    const long long chunk = std::max<long long>(1, std::min<long long>(std::min<long long>(batch, 65535),
                                                                       TTN_ZMEASURE_CHUNK_BYTES / (long long)(sizeof(double) * M.per_train)));
    int rc;
    if ((rc = scratch_take(sizeof(double) * (size_t)M.per_train * (size_t)chunk))) return rc;
    if ((rc = g_zmeasure_tab.ensure(sizeof(double) * g_zmeasure_host.size()))) return rc;
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    HIPCHK(hipMemcpyAsync(g_zmeasure_tab.p, g_zmeasure_host.data(), sizeof(double) * g_zmeasure_host.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipEventRecord(g_zmeasure_ev, g_stream));
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, batch - b0);
        ZMeasureArgs P;
        memset(&P, 0, sizeof(P));
        P.x = x->dev();
        P.x.data += b0 * x->stride; P.x.rks += b0 * (d + 1); P.x.batch = nb;
        P.env = g_scratch.as<double>(); P.W = M.W;
        P.toff = g_zmeasure_tab.as<long long>();
        P.tabs = g_zmeasure_tab.as<double>() + d;
        P.S = M.S; P.ntab = ntab;
        P.V = P.env + (size_t)2 * (d + 1) * M.W * nb;
        P.St = P.V + (size_t)ntab * d * M.W * nb;
        P.ctb = P.St + (size_t)npass * (d - 1) * 2 * M.W * nb;
        P.work = P.ctb + (size_t)2 * M.N * nb;
        P.tsz = M.N; P.wstride = 2 * M.N;
        P.out = d_out + 2 * b0 * ob;
        P.ob = ob; P.ot = ot; P.ok = ok; P.nemit = nemit;
        P.normalize = normalize ? 1 : 0;
        for (int p = 0; p < npass; ++p) { P.o1[p] = o1[p]; P.o2[p] = o2[p]; }
        P.mirror = mirror ? 1 : 0;
        P.skip_fit = M.chip ? 1 : 0;
        if (M.chip) zmeasure_phases<true>(P, d, nb, ntab, npass);
        if (M.gen) zmeasure_phases<false>(P, d, nb, ntab, npass);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    return TTN_OK;
}

static int zsite_expect_launch(const char* who, ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out) {
    if (nops < 1 || nops > TTN_ZMEASURE_MAX_OPS) return fail(TTN_ERR_ARG, (std::string(who) + ": nops must be in 1:16").c_str());
    ZMeasurePlan M;
    int rc;
    if ((rc = zmeasure_plan(who, x, (int)nops, 0, M))) return rc;
    std::vector<const double*> tabs((size_t)nops);
    for (int64_t t = 0; t < nops; ++t) tabs[t] = ops + t * 2 * M.S;
    return zmeasure_run(x, M, (int)nops, tabs.data(), (int)nops, (long long)x->d * nops, x->d, 1, 0, nullptr, nullptr, false, normalize, d_out);
}

int ttn_zsite_expect_dev(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !ops || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    return zsite_expect_launch("ttn_zsite_expect_dev", x, nops, ops, normalize, d_out);
}

int ttn_zsite_expect(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !ops || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (nops < 1 || nops > TTN_ZMEASURE_MAX_OPS) return fail(TTN_ERR_ARG, "ttn_zsite_expect: nops must be in 1:16");
    const size_t bytes = sizeof(double) * 2 * (size_t)x->d * (size_t)nops * (size_t)x->batch;
    int rc;
    { ZMeasurePlan M; if ((rc = zmeasure_plan("ttn_zsite_expect", x, (int)nops, 0, M))) return rc; }      // every check before the first allocation
    if ((rc = g_dout.ensure(bytes))) return rc;
    if ((rc = zsite_expect_launch("ttn_zsite_expect", x, nops, ops, normalize, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, bytes, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// Tables of a correlation: 0 = P_k Q_k (the diagonal, built here), 1 = P, 2 = Q (absent when Q equals P bitwise).
static int zcorrelation_launch(const char* who, ttn_tt_t x, const double* Pt, const double* Qt, int64_t normalize, double* d_out) {
    ZMeasurePlan M;
    int rc;
    if ((rc = zmeasure_plan(who, x, 3, 2, M))) return rc;
    const int d = x->d;
    const bool same = Pt == Qt || memcmp(Pt, Qt, sizeof(double) * 2 * (size_t)M.S) == 0;
    if (same) { M = ZMeasurePlan(); if ((rc = zmeasure_plan(who, x, 2, 1, M))) return rc; }
    std::vector<double> PQ(2 * (size_t)M.S);
    {
        size_t off = 0;
        for (int k = 0; k < d; ++k) {
            const int n = (int)x->dims[k];
            for (int c = 0; c < n; ++c)
                for (int r = 0; r < n; ++r) {
                    double ar = 0.0, ai = 0.0;
                    for (int w = 0; w < n; ++w) {
                        const double* p = Pt + 2 * (off + r + (size_t)n * w);
                        const double* q = Qt + 2 * (off + w + (size_t)n * c);
                        ar += p[0] * q[0] - p[1] * q[1];
                        ai += p[0] * q[1] + p[1] * q[0];
                    }
                    PQ[2 * (off + r + (size_t)n * c)] = ar;
                    PQ[2 * (off + r + (size_t)n * c) + 1] = ai;
                }
            off += (size_t)n * n;
        }
    }
    const double* tabs[3] = {PQ.data(), Pt, Qt};
    const int o1[2] = {same ? 1 : 2, 1}, o2[2] = {1, 2};              // pass 0: (O1, O2) = (Q, P), the upper triangle; pass 1: (P, Q), the lower
    return zmeasure_run(x, M, same ? 2 : 3, tabs, 1, (long long)d * d, 0, d + 1, same ? 1 : 2, o1, o2, same, normalize, d_out);
}

int ttn_zcorrelation_dev(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !P || !Q || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    return zcorrelation_launch("ttn_zcorrelation_dev", x, P, Q, normalize, d_out);
}

int ttn_zcorrelation(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !P || !Q || !out) return fail(TTN_ERR_ARG, "null pointer");
    const size_t bytes = sizeof(double) * 2 * (size_t)x->d * (size_t)x->d * (size_t)x->batch;
    int rc;
    { ZMeasurePlan M; if ((rc = zmeasure_plan("ttn_zcorrelation", x, 3, 2, M))) return rc; }
    if ((rc = g_dout.ensure(bytes))) return rc;
    if ((rc = zcorrelation_launch("ttn_zcorrelation", x, P, Q, normalize, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, bytes, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_ZMEASURE_H
