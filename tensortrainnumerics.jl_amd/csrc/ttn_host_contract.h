// ttn_host_contract.h — host API: partial contraction of resident trains (include/ttn_contract.h, csrc/ttn_contract_kernels.h).
#ifndef TTN_HOST_CONTRACT_H
#define TTN_HOST_CONTRACT_H
#include "ttn_host_core.h"
#include "ttn_contract_kernels.h"

namespace {
std::vector<double> g_contract_host;    // the host copy of the tables of the last ttn_tt_contract_sites, untouched until its upload has completed
hipEvent_t g_contract_ev = nullptr;
DevBuf g_contract_tab;     // [d] weight offsets, the weight tables, then kept / start / the three launch lists as ints
}  // namespace

extern "C" {
// ---- partial contraction ------------------------------------------------------------------------------------------
int ttn_tt_contract_sites(ttn_tt_t x, int64_t ncontract, const int64_t* sites, int64_t wbatch, const double* weights, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    const char* who = "ttn_tt_contract_sites";
    if (!x || !y || !sites || !weights) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: null handle or pointer");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: output must not alias the input");
    F64_ONLY(who, {x, y});
    const int d = x->d, batch = x->batch;
    if (ncontract < 1) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: no site to contract (ttn_tt_copy copies a train)");
    if (ncontract > d) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: more sites than the train has (a site is repeated or out of range)");
    std::vector<char> contracted((size_t)d, 0);
    for (int64_t j = 0; j < ncontract; ++j) {
        if (sites[j] < 1 || sites[j] > d) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: site out of range (sites are 1-based)");
        if (j && sites[j] <= sites[j - 1]) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: sites must be strictly increasing");
        contracted[(size_t)sites[j] - 1] = 1;
    }
    if (ncontract == d) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: no kept site (a full contraction is ttn_dot with the rank-1 train of the weights)");
    if (wbatch != 1 && wbatch != batch) return fail(TTN_ERR_ARG, "ttn_tt_contract_sites: wbatch must be 1 or the batch size");
    const int K = d - (int)ncontract;
    std::vector<int> kept, start;
    for (int k = 0, run = 0; k < d; ++k)
        if (!contracted[k]) { kept.push_back(k); start.push_back(run); run = k + 1; }
    if (y->d != K) return fail(TTN_ERR_DIMS, "ttn_tt_contract_sites: the destination must have one site per kept site");
    for (int m = 0; m < K; ++m)
        if (y->dims[m] != x->dims[kept[m]]) return fail(TTN_ERR_DIMS, "ttn_tt_contract_sites: the destination's dimensions are not those of the kept sites");
    if (y->batch != batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (x->bound[0] != 1 || x->bound[d] != 1) return fail(TTN_ERR_DIMS, "ttn_tt_contract_sites: the input must have end ranks 1");
    std::vector<int64_t> yb((size_t)K + 1);
    for (int m = 0; m < K; ++m) yb[m] = x->bound[start[m]];
    yb[K] = x->bound[d];
    for (int m = 0; m <= K; ++m) if (y->cap[m] < yb[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_contract_sites: destination capacity too small");
    for (const ttn_tt_s* h : {(const ttn_tt_s*)x, (const ttn_tt_s*)y})
        for (int k = 0; k < h->d; ++k)
            if (h->off[k + 1] - h->off[k] >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_contract_sites: a core of 2^31 doubles or more (32-bit element indices)");

    // the three launches: copies, vector chains, matrix chains (on chip or general)
    long long rcap = 1, ncap = 1, xcap = 1;
    bool chip = true;
    for (int m = 0; m <= d; ++m) { rcap = std::max<long long>(rcap, x->bound[m]); xcap = std::max<long long>(xcap, x->cap[m]); }
    for (int k = 0; k < d; ++k) { ncap = std::max<long long>(ncap, x->dims[k]); chip = chip && x->dims[k] == 2; }
    chip = chip && xcap <= CONTRACT_RMAX;
    std::vector<int> lcopy, lvec, lmat;
    for (int m = 0; m < K; ++m) {
        const bool lead = start[m] < kept[m], trail = m == K - 1 && kept[m] < d - 1;
        if (!lead && !trail) lcopy.push_back(m);
        else if (!lead || start[m] == 0) lvec.push_back(m);
        else lmat.push_back(m);
    }
    const long long wv = (4 * rcap + ncap * rcap + 1) & ~1LL;
    const long long wm = chip ? 0 : (3 * rcap * rcap + 2 * rcap + ncap * rcap + 1) & ~1LL;
    const long long per_train = (long long)lvec.size() * wv + (long long)lmat.size() * wm;
    long long chunk = std::min<long long>(batch, 65535);
    if (per_train > 0) chunk = std::max<long long>(1, std::min<long long>(chunk, TTN_CONTRACT_CHUNK_BYTES / (long long)(sizeof(double) * per_train)));

    // the tables travel from a host copy that stays untouched until the upload has completed
    long long S = 0;
    std::vector<long long> woff((size_t)d, 0);
    for (int64_t j = 0; j < ncontract; ++j) { woff[(size_t)sites[j] - 1] = S; S += x->dims[(size_t)sites[j] - 1]; }
    if (!g_contract_ev) HIPCHK(hipEventCreateWithFlags(&g_contract_ev, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(g_contract_ev));
    const size_t wtot = (size_t)wbatch * (size_t)S, nint = 3 * (size_t)K;
    g_contract_host.assign((size_t)d + wtot + (nint + 1) / 2, 0.0);
    memcpy(g_contract_host.data(), woff.data(), sizeof(long long) * (size_t)d);
    memcpy(g_contract_host.data() + d, weights, sizeof(double) * wtot);
    {
        int* ip = reinterpret_cast<int*>(g_contract_host.data() + d + wtot);
        memcpy(ip, kept.data(), sizeof(int) * (size_t)K);
        memcpy(ip + K, start.data(), sizeof(int) * (size_t)K);
        int* lp = ip + 2 * K;
        for (const std::vector<int>* l : {&lcopy, &lvec, &lmat}) { if (!l->empty()) memcpy(lp, l->data(), sizeof(int) * l->size()); lp += l->size(); }
    }
    int rc;
    if ((rc = scratch_take(std::max<size_t>(16, sizeof(double) * (size_t)per_train * (size_t)chunk)))) return rc;
    if ((rc = g_contract_tab.ensure(sizeof(double) * g_contract_host.size()))) return rc;
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    HIPCHK(hipMemcpyAsync(g_contract_tab.p, g_contract_host.data(), sizeof(double) * g_contract_host.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipEventRecord(g_contract_ev, g_stream));
    y->bound = yb;
    std::fill(y->ot.begin(), y->ot.end(), 0);
    const int* d_int = reinterpret_cast<const int*>(g_contract_tab.as<double>() + d + wtot);
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, batch - b0);
        ContractArgs A;
        A.x = x->dev(); A.x.data += b0 * x->stride; A.x.rks += b0 * (d + 1); A.x.batch = nb;
        A.y = y->dev(); A.y.data += b0 * y->stride; A.y.rks += b0 * (K + 1); A.y.batch = nb;
        A.kept = d_int; A.start = d_int + K; A.list = d_int + 2 * K;
        A.woff = g_contract_tab.as<long long>();
        A.wstride = wbatch == 1 ? 0 : S;
        A.w = g_contract_tab.as<double>() + d + b0 * A.wstride;
        A.work = g_scratch.as<double>(); A.wsz = 0;
        A.rcap = (int)rcap; A.ncap = (int)ncap; A.K = K;
        hipLaunchKernelGGL(k_contract_ranks, dim3(nb), dim3(64), 0, g_stream, A);
        HIPCHK(hipGetLastError());
        if (!lcopy.empty()) {
            hipLaunchKernelGGL(k_contract_copy, dim3((unsigned)lcopy.size(), nb), dim3(CONTRACT_COPY_TB), 0, g_stream, A);
            HIPCHK(hipGetLastError());
        }
        A.list += lcopy.size();
        if (!lvec.empty()) {
            A.wsz = wv;
            hipLaunchKernelGGL(k_contract_vec, dim3((unsigned)lvec.size(), nb), dim3(CONTRACT_VEC_TB), 0, g_stream, A);
            HIPCHK(hipGetLastError());
        }
        A.list += lvec.size();
        if (!lmat.empty()) {
            A.work += (long long)lvec.size() * wv * nb; A.wsz = wm;
            if (chip) hipLaunchKernelGGL(k_contract_chip, dim3((unsigned)lmat.size(), nb), dim3(CONTRACT_CHIP_TB), CONTRACT_CHIP_LDS_BYTES, g_stream, A);
            else hipLaunchKernelGGL(k_contract_gen, dim3((unsigned)lmat.size(), nb), dim3(TTN_WG), sizeof(double) * GEMM_LDS_TOTAL, g_stream, A);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_CONTRACT_H
