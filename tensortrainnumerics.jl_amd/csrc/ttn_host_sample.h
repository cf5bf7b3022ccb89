// ttn_host_sample.h — host API: sampling.
#ifndef TTN_HOST_SAMPLE_H
#define TTN_HOST_SAMPLE_H
#include "ttn_host_core.h"
#include "ttn_dot_kernels.h"
#include "ttn_grad_kernels.h"
#include "ttn_sample_kernels.h"

namespace {
std::vector<hipEvent_t> g_sample_ev;    // ttn_tt_sample, three per chunk of trains: before the environments, between the phases, after the sweeps
int g_sample_chunks = 0;                // chunks of the last call (0: none has run)
DevBuf g_sample_out;       // device outputs of the host form ttn_tt_sample: indices, log-probabilities, info words
}  // namespace

extern "C" {
// ---- sampling (include/ttn_sample.h, csrc/ttn_sample_kernels.h) ----------------------------------------------------------
static_assert(SAMPLE_TILE == TTN_SAMPLE_TILE, "ttn_sample.h and ttn_sample_kernels.h disagree");
// What one train needs for its environments and one tile of samples for the general route's products (doubles), checked before anything
// is launched.
struct SamplePlan {
    long long W = 1, tsz = 1, gss = 1, per_train = 0, per_tile = 0, vsz = 0, wsz = 0;
    bool born = true;
};
static int sample_plan(const char* who, const ttn_tt_s* x, int64_t mode, int64_t nsamples, SamplePlan& M) {
    const std::string w(who);
    if (nsamples < 1) return fail(TTN_ERR_ARG, (w + ": nsamples must be at least 1").c_str());
    if (mode != TTN_SAMPLE_BORN && mode != TTN_SAMPLE_DENSITY) return fail(TTN_ERR_ARG, (w + ": mode must be TTN_SAMPLE_BORN (0) or TTN_SAMPLE_DENSITY (1)").c_str());
    F64_ONLY(who, {x});
    const int d = x->d;
    if (d > SAMPLE_MAX_D) return fail(TTN_ERR_UNSUPPORTED, (w + ": chains longer than 480 sites are not supported").c_str());
    if (x->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + ": a train of 2^31 doubles or more").c_str());
    long long rmax = 1, nmax = 1;
    bool gen = false;
    for (int m = 0; m <= d; ++m) rmax = std::max<long long>(rmax, x->bound[m]);
    for (int k = 0; k < d; ++k) {
        nmax = std::max<long long>(nmax, x->dims[k]);
        gen = gen || x->dims[k] != 2;
    }
    gen = gen || rmax > DOT_RMAX;
    const char* big = ": ranks too large (the workspace of one train reaches 2^31 doubles)";
    if (rmax >= (1LL << 16) || nmax >= (1LL << 31) || nmax * rmax * rmax >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    M.born = mode == TTN_SAMPLE_BORN;
    M.W = (rmax * rmax + 1) & ~1LL;
    M.tsz = (nmax * rmax * rmax + 1) & ~1LL;
    M.gss = M.born ? M.W : ((rmax + 1) & ~1LL);
    M.per_train = M.born ? 2 * (d + 1) * M.W + 2 * M.tsz : (d + 1) * M.gss;
    M.vsz = gen ? SAMPLE_TILE * rmax : 0;
    M.wsz = gen ? SAMPLE_TILE * nmax * rmax : 0;
    M.per_tile = gen ? M.vsz + 2 * M.wsz + SAMPLE_TILE * nmax : 0;
    if (M.per_train + M.per_tile >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (w + big).c_str());
    return TTN_OK;
}

static int sample_run(ttn_tt_t x, const SamplePlan& M, int64_t nsamples, int64_t seed, const double* d_u, int64_t* d_idx, double* d_logp, int64_t* d_info) {
    const int d = x->d, batch = x->batch;
    const long long S = nsamples, budget = TTN_SAMPLE_CHUNK_BYTES / (long long)sizeof(double);
    // trains per chunk: their environments take at most half the bound; tiles per launch: what the rest holds (one at least)
    const long long chunk = std::max<long long>(1, std::min<long long>(std::min<long long>(batch, 65535), budget / 2 / M.per_train));
    const long long tiles_all = (S + SAMPLE_TILE - 1) / SAMPLE_TILE;
    long long tiles = std::min<long long>(tiles_all, 1LL << 20);
    if (M.per_tile) tiles = std::max<long long>(1, std::min<long long>(tiles, (budget - chunk * M.per_train) / (chunk * M.per_tile)));
    int rc;
    if ((rc = scratch_take(sizeof(double) * (size_t)(chunk * M.per_train + chunk * tiles * M.per_tile)))) return rc;
    int nchunks = 0;
    if (d_info) HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int64_t) * 2 * (size_t)batch, g_stream));
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, batch - b0);
        TTDev xd = x->dev();
        xd.data += b0 * x->stride; xd.rks += b0 * (d + 1); xd.batch = nb;
        double* env = g_scratch.as<double>();
        while (g_sample_ev.size() < (size_t)3 * (nchunks + 1)) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            g_sample_ev.push_back(e);
        }
        hipEvent_t* ev = &g_sample_ev[(size_t)3 * nchunks++];
        HIPCHK(hipEventRecord(ev[0], g_stream));
        SampleArgs P;
        memset(&P, 0, sizeof(P));
        if (M.born) {
            GradChainArgs C_;
            C_.a = xd; C_.b = xd;
            C_.env = env;
            C_.tbuf = env + (size_t)2 * (d + 1) * M.W * nb;
            C_.W = M.W; C_.tsz = M.tsz;
            C_.out = nullptr;
            hipLaunchKernelGGL(k_grad_chain, dim3(nb, 2), dim3(TTN_WG), DOT_LDS_BYTES(d), g_stream, C_);
            HIPCHK(hipGetLastError());
            P.genv = env + (size_t)(d + 1) * M.W;                         // the G half of train 0: G_1 .. G_{d+1}
            P.gbs = 2 * (d + 1) * M.W; P.gss = M.W;
        } else {
            SampleEnvArgs E_;
            E_.x = xd; E_.g = env; E_.gbs = (d + 1) * M.gss; E_.gss = M.gss;
            hipLaunchKernelGGL(k_sample_genv, dim3(nb), dim3(TTN_WG), 0, g_stream, E_);
            HIPCHK(hipGetLastError());
            P.genv = env; P.gbs = E_.gbs; P.gss = M.gss;
        }
        HIPCHK(hipEventRecord(ev[1], g_stream));
        P.x = xd;
        P.born = M.born ? 1 : 0;
        P.S = S;
        P.seed = (unsigned long long)seed;
        P.b0 = b0;
        P.u = d_u ? d_u + (size_t)b0 * S * d : nullptr;
        P.idx = (long long*)d_idx + (size_t)b0 * S * d;
        P.logp = d_logp + (size_t)b0 * S;
        P.info = d_info ? (unsigned long long*)d_info + 2 * b0 : nullptr;
        P.work = env + (size_t)M.per_train * nb;
        P.wstride = M.per_tile; P.vsz = M.vsz; P.wsz = M.wsz;
        for (long long t0 = 0; t0 < tiles_all; t0 += tiles) {
            const long long nt = std::min<long long>(tiles, tiles_all - t0);
            P.s0 = t0 * SAMPLE_TILE;
            P.s1 = std::min<long long>(S, (t0 + nt) * SAMPLE_TILE);
            hipLaunchKernelGGL(k_sample_sweep, dim3((unsigned)nt, nb), dim3(TTN_WG), SAMPLE_LDS_BYTES, g_stream, P);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ev[2], g_stream));
    }
    g_sample_chunks = nchunks;
    return TTN_OK;
}

int ttn_tt_sample_dev(ttn_tt_t x, int64_t mode, int64_t nsamples, int64_t seed, const double* d_u, int64_t* d_idx, double* d_logp, int64_t* d_info) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !d_idx || !d_logp) return fail(TTN_ERR_ARG, "null pointer");
    SamplePlan M;
    int rc;
    if ((rc = sample_plan("ttn_tt_sample_dev", x, mode, nsamples, M))) return rc;
    return sample_run(x, M, nsamples, seed, d_u, d_idx, d_logp, d_info);
}

int ttn_tt_sample(ttn_tt_t x, int64_t mode, int64_t nsamples, int64_t seed, const double* d_u, int64_t* idx, double* logp, int64_t* info) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !idx || !logp) return fail(TTN_ERR_ARG, "null pointer");
    SamplePlan M;
    int rc;
    if ((rc = sample_plan("ttn_tt_sample", x, mode, nsamples, M))) return rc;         // every check before the first allocation
    const size_t rows = (size_t)x->batch * (size_t)nsamples;
    const size_t b_idx = sizeof(int64_t) * rows * (size_t)x->d, b_lp = sizeof(double) * rows, b_info = sizeof(int64_t) * 2 * (size_t)x->batch;
    if ((rc = g_sample_out.ensure(b_idx + b_lp + b_info))) return rc;
    int64_t* d_idx = g_sample_out.as<int64_t>();
    double* d_logp = (double*)((char*)g_sample_out.p + b_idx);
    int64_t* d_info = (int64_t*)((char*)g_sample_out.p + b_idx + b_lp);
    if ((rc = sample_run(x, M, nsamples, seed, d_u, d_idx, d_logp, d_info))) return rc;
    HIPCHK(hipMemcpyAsync(idx, d_idx, b_idx, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(logp, d_logp, b_lp, hipMemcpyDeviceToHost, g_stream));
    if (info) HIPCHK(hipMemcpyAsync(info, d_info, b_info, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

int ttn_tt_sample_last_ms(double* env_ms, double* sweep_ms) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!env_ms || !sweep_ms) return fail(TTN_ERR_ARG, "null pointer");
    if (!g_sample_chunks) return fail(TTN_ERR_ARG, "ttn_tt_sample_last_ms: no ttn_tt_sample call has run");
    HIPCHK(hipEventSynchronize(g_sample_ev[(size_t)3 * g_sample_chunks - 1]));
    double a = 0.0, b = 0.0;
    for (int c = 0; c < g_sample_chunks; ++c) {
        float fa = 0.f, fb = 0.f;
        HIPCHK(hipEventElapsedTime(&fa, g_sample_ev[3 * c], g_sample_ev[3 * c + 1]));
        HIPCHK(hipEventElapsedTime(&fb, g_sample_ev[3 * c + 1], g_sample_ev[3 * c + 2]));
        a += fa; b += fb;
    }
    *env_ms = a; *sweep_ms = b;
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_SAMPLE_H
