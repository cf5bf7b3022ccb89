// ttn_api.hip — the C ABI of include/ttn.h on top of the HIP kernels (gfx950).
// The host code is being cut into csrc/ttn_host_*.h, one header per feature (ttn_host_core.h describes the layering); what is not
// cut yet stands below, in the order it always had, and ttn_init / ttn_finalize stand last because they see every module's state.
// There is no block of globals: state that one feature alone uses is declared with that feature, here as in the host headers.
//
// The kernel headers.  Their order here is the order of the kernels in the code object: do not "tidy" it (sort it, or drop an
// include because a host header pulls it in) — the device code would no longer be byte-identical to the build before.
#include "../../include/ttn.h"
#include "ttn_common.h"
#include "ttn_stream_kernels.h"
#include "ttn_dense_kernels.h"
#include "ttn_swap_kernels.h"
#include "ttn_selftest_kernels.h"
#include "ttn_dot_kernels.h"
#include "ttn_ortho_kernels.h"
#include "ttn_ortho512.h"
#include "ttn_ortho_ramp.h"
#include "ttn_hsvd_kernels.h"
#include "ttn_resite_kernels.h"
#include "ttn_als_kernels.h"
#include "ttn_als_grid.h"
#include "ttn_eigsolve_kernels.h"
#include "ttn_eig_ortho_kernels.h"
#include "ttn_als_eig_kernels.h"
#include "ttn_eig_kernels.h"
#include "ttn_tdvp_kernels.h"
#include "ttn_densefact_kernels.h"
#include "ttn_cross_kernels.h"
#include "ttn_cross_batch_kernels.h"
#include "ttn_opalg_kernels.h"
#include "ttn_cplx_kernels.h"
#include "ttn_grid_kernels.h"
#include "ttn_grad_kernels.h"
#include "ttn_rect_kernels.h"
#include "ttn_step_kernels.h"
#include "ttn_expect_kernels.h"
#include "ttn_expect_grad_kernels.h"
#include "ttn_opbatch_kernels.h"
#include "ttn_measure_kernels.h"
#include "ttn_sample_kernels.h"
#include "ttn_braket_kernels.h"
#include "ttn_tangent_kernels.h"
#include "ttn_contract_kernels.h"
#include "ttn_zmeasure_kernels.h"

// The host headers: the dynamic-LDS table first (it fixes the order of the kernel templates' instantiations, see there), then the
// layers, lowest first — every header stands after the ones it includes (tests/test_cpu_headers.py).
#include "ttn_host_lds.h"
#include "ttn_host_core.h"
#include "ttn_host_dot.h"
#include "ttn_host_measure.h"
#include "ttn_host_sample.h"
#include "ttn_host_handles.h"
#include "ttn_host_stream.h"
#include "ttn_host_rect.h"
#include "ttn_host_compress.h"
#include "ttn_host_braket.h"
#include "ttn_host_tangent.h"
#include "ttn_host_contract.h"
#include "ttn_host_zmeasure.h"

// the 512-thread build of k_compress and its building blocks (ttn_wg512.hip: two workgroups per CU), declared once for both units
#include "ttn_wg512.h"

extern "C" {

// ---- site-swap chains: hadamard_ttm and reorder -----------------------------------------------------
// Launch of k_swap_chain.  `ops` = (type, slotA, slotB) triples; kind 1 works in an arena of 2d uniform slots carved out of
// the scratch allocation, kind 2 in place on the handle's own slots.
static int launch_chain(int kind, ttn_tt_t x, ttn_tt_t y, ttn_tt_t z, int n, int nslots, int64_t work_cap, const std::vector<int>& ops,
                        const std::vector<int>& final_slots, double tol, int64_t rmax, int rank_rule) {
    ttn_tt_t ref = (kind == 1) ? x : z;
    const int batch = ref->batch;
    const long long pmax = (long long)n * work_cap, qmax = pmax;
    if (pmax > 256) return fail(TTN_ERR_UNSUPPORTED, "site-swap chain: n * rank capacity must be <= 256");
    const long long per_compress = 2 * pmax * qmax + QR_NB * qmax + pmax * QR_NB + 2 * pmax * pmax + 4 * pmax + 64 + 6 * 128 * 128;
    const long long slot_doubles = (kind == 1) ? (long long)n * work_cap * work_cap : 0;
    const long long srk_stride = 2 * nslots + 2;
    const long long per_train = per_compress + srk_stride + (long long)nslots * slot_doubles;
    const size_t tab_ints = ops.size() + final_slots.size();
    int rc = scratch_take(sizeof(double) * (size_t)per_train * batch + sizeof(int) * tab_ints + 64);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * batch);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    int* d_tab = (int*)(base + (size_t)per_train * batch);
    std::vector<int> h_tab(ops);
    h_tab.insert(h_tab.end(), final_slots.begin(), final_slots.end());
    HIPCHK(hipMemcpyAsync(d_tab, h_tab.data(), sizeof(int) * tab_ints, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));            // h_tab is a local
    ChainArgs Q;
    memset(&Q, 0, sizeof(Q));
    CompressArgs& P = Q.C;
    if (kind == 2) P.tt = z->dev();
    P.max_bond = rmax;
    P.truncerr = tol;
    P.sweeps = 1;
    P.scratch = base;
    P.scratch_stride = per_train;
    P.pmax = (int)pmax; P.qmax = (int)qmax;
    P.sv_out = nullptr; P.sv_steps = 0;
    P.status = z->d_status;                 // the handle the chain writes (kind 2: in place on z)
    P.sweep_stats = z->d_status + batch;
    P.fast = 0;
    P.fused = 0;
    P.rank_rule = rank_rule;
    Q.kind = kind;
    Q.n = n; Q.nslots = nslots; Q.nops = (int)(ops.size() / 3); Q.d = (kind == 1) ? x->d : z->d;
    Q.ops = d_tab;
    Q.final_slots = d_tab + ops.size();
    Q.arena = base + per_compress + srk_stride;        // per train: [compress scratch | slot ranks | slots]
    Q.arena_stride = per_train;
    Q.slot_doubles = slot_doubles;
    Q.cap = (int)work_cap;
    Q.srk = (long long*)(base + per_compress);
    Q.srk_stride = per_train;                           // in units of 8 bytes, like the doubles
    if (kind == 1) { Q.x = x->dev(); Q.y = y->dev(); Q.z = z->dev(); }
    hipLaunchKernelGGL(k_swap_chain, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Q);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_hadamard_ttm(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z, double tol, int64_t rmax, int64_t work_cap) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_hadamard_ttm", {x, y, z});
    if (!x || !y || !z) return fail(TTN_ERR_ARG, "null handle");
    if (!same_dims(x->dims, y->dims) || !same_dims(x->dims, z->dims)) return fail(TTN_ERR_DIMS, "Incompatible TT dimensions");
    if (x->batch != y->batch || x->batch != z->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (z == x || z == y) return fail(TTN_ERR_ARG, "ttn_hadamard_ttm: output must not alias an input");
    if (rmax < 1 || work_cap < 1 || tol < 0.0) return fail(TTN_ERR_ARG, "bad tol / rmax / work_cap");
    const int d = x->d;
    const int64_t n = x->dims[0];
    for (int k = 0; k < d; ++k) if (x->dims[k] != n) return fail(TTN_ERR_UNSUPPORTED, "ttn_hadamard_ttm: all physical dimensions must be equal");
    if (2 * d > 2 * TTN_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "chain too long");
    for (int m = 0; m <= d; ++m)
        if (x->bound[m] > work_cap || y->bound[m] > work_cap) return fail(TTN_ERR_CAPACITY, "ttn_hadamard_ttm: work_cap below an input rank");
    // the reference's loops (tt_operations.jl:414-420) as ops on fixed slots.  With L0 = 2d (iter 1) or d-iter+2 (later) the
    // logical core l (1-based) lives in slot l (l <= L0) or l - L0 + d + 1: the contraction of iteration i frees slot d+2-i.
    std::vector<int> ops, fin;
    auto slot = [&](int iter, int l) { const int L0 = (iter == 1) ? 2 * d : d - iter + 2; return (l <= L0 ? l : l - L0 + d + 1) - 1; };
    for (int iter = 1; iter <= d; ++iter) {
        for (int j = d; j >= d - iter + 2; --j) { ops.push_back(0); ops.push_back(slot(iter, j)); ops.push_back(slot(iter, j + 1)); }
        const int pc = d - iter + 1;
        ops.push_back(1); ops.push_back(slot(iter, pc)); ops.push_back(slot(iter, pc + 1));
    }
    for (int l = 1; l <= d; ++l) fin.push_back(slot(d + 1, l));
    int rc = launch_chain(1, x, y, z, (int)n, 2 * d, work_cap, ops, fin, tol, rmax, 0);
    if (rc) return rc;
    for (int m = 0; m <= d; ++m) z->bound[m] = std::min<int64_t>(z->cap[m], std::min<int64_t>(work_cap, rmax));
    z->bound[0] = 1; z->bound[d] = 1;
    std::fill(z->ot.begin(), z->ot.end(), 0);
    return TTN_OK;
}

int ttn_swap_sites(ttn_tt_t x, int64_t nswaps, const int64_t* swaps, double threshold) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_swap_sites", {x});
    if (!x || nswaps < 0 || (nswaps > 0 && !swaps) || threshold < 0.0) return fail(TTN_ERR_ARG, "bad argument");
    const int d = x->d;
    const int64_t n = x->dims[0];
    for (int k = 0; k < d; ++k) if (x->dims[k] != n) return fail(TTN_ERR_UNSUPPORTED, "ttn_swap_sites: all physical dimensions must be equal");
    int64_t capmax = 1;
    for (int m = 0; m <= d; ++m) capmax = std::max(capmax, x->cap[m]);
    std::vector<int> ops, fin;
    std::vector<int64_t> bnd = x->bound;
    for (int64_t i = 0; i < nswaps; ++i) {
        const int64_t k = swaps[i];
        if (k < 1 || k >= d) return fail(TTN_ERR_BOND_INDEX, "k must be in 1:(N-1)");
        // length(F.S) = min(n r_{k-1}, n r_{k+1}) is kept whole when threshold == 0 (qtt_tools.jl:681-685)
        const int64_t full = std::min(n * bnd[k - 1], n * bnd[k + 1]);
        if (threshold == 0.0 && full > x->cap[k]) return fail(TTN_ERR_CAPACITY, "ttn_swap_sites: a bond rank grows beyond the handle's capacity");
        bnd[k] = std::min(full, x->cap[k]);
        ops.push_back(0); ops.push_back((int)k - 1); ops.push_back((int)k);
    }
    if (nswaps == 0) return TTN_OK;
    int rc = launch_chain(2, nullptr, nullptr, x, (int)n, d, capmax, ops, fin, threshold, (int64_t)1 << 62, 1);
    if (rc) return rc;
    x->bound = bnd;
    std::fill(x->ot.begin(), x->ot.end(), 0);
    return TTN_OK;
}

// ---- ttv_decomp: dense tensors -> trains ----------------------------------------------------------------
// The size checks of a decomposition into d sites `dims` with rank capacities `cap`, rooted at `index` (1-based), and what they compute:
// the host-side rank bounds and the worst-case short / long sides of the unfoldings.  The messages name `who`; `hint` says how the caller
// lowers the capacities.
static int ttv_decomp_plan(const char* who, const char* hint, int d, const int64_t* dims, const int64_t* cap, int64_t index, std::vector<int64_t>& bnd,
                           long long& total, long long& pmax, long long& qmax) {
    if (index < 1 || index > d) return fail(TTN_ERR_ARG, "index must be in 1:d");
    total = 1;
    for (int k = 0; k < d; ++k) {
        total *= dims[k];
        if (total > (1LL << 27)) return fail(TTN_ERR_UNSUPPORTED, (std::string(who) + ": more than 2^27 entries per tensor").c_str());
    }
    // worst-case short / long sides of the unfoldings, with the ranks bounded by the handle's capacity
    bnd.assign(d + 1, 1);
    pmax = 1; qmax = 1;
    {
        long long len = total, rl = 1;
        for (int i = 0; i < index - 1; ++i) {
            const long long a = rl * dims[i], bc = len / a;
            pmax = std::max(pmax, std::min(a, bc)); qmax = std::max(qmax, std::max(a, bc));
            rl = std::min<long long>(std::min(a, bc), cap[i + 1]);
            bnd[i + 1] = rl; len = rl * bc;
        }
        long long rr = 1;
        for (int i = d - 1; i > index - 1; --i) {
            const long long a = dims[i] * rr, rows = len / a;
            pmax = std::max(pmax, std::min(a, rows)); qmax = std::max(qmax, std::max(a, rows));
            rr = std::min<long long>(std::min(a, rows), cap[i]);
            bnd[i] = rr; len = rows * rr;
        }
    }
    if (pmax > 4096) return fail(TTN_ERR_UNSUPPORTED, (std::string(who) + ": an unfolding has a short side above 4096 (" + hint + ")").c_str());
    return TTN_OK;
}

// One body for both entry points: `on_device` says where `tensors` lives.  HOST tensors are copied behind the working buffers; DEVICE
// tensors are read in place (k_ttv_decomp only reads them: its first step copies train b's tensor into its own working buffer).
static int ttv_decomp_impl(ttn_tt_t z, const double* tensors, int64_t index, double tol, bool on_device) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY(on_device ? "ttn_ttv_decomp_dev" : "ttn_ttv_decomp", {z});
    if (!z || !tensors) return fail(TTN_ERR_ARG, "null argument");
    const int d = z->d;
    std::vector<int64_t> bnd;
    long long total, pmax, qmax;
    { const int rc = ttv_decomp_plan("ttn_ttv_decomp", "lower the handle's rank capacity", d, z->dims.data(), z->cap.data(), index, bnd, total, pmax, qmax); if (rc) return rc; }
    const long long per_scr = QR_NB * qmax + pmax * QR_NB + 2 * pmax * pmax + 4 * pmax + 64;
    const long long per_train = 3 * total + per_scr;
    const int batch = z->batch;
    int rc = scratch_take(sizeof(double) * ((size_t)per_train * batch + (on_device ? 0 : (size_t)total * batch)));
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * batch);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    const double* d_in = tensors;
    if (!on_device) {
        double* stage = base + (size_t)per_train * batch;
        HIPCHK(hipMemcpyAsync(stage, tensors, sizeof(double) * (size_t)total * batch, hipMemcpyHostToDevice, g_stream));
        d_in = stage;
    }
    HsvdArgs H;
    memset(&H, 0, sizeof(H));
    CompressArgs& P = H.C;
    P.tt = z->dev();
    P.max_bond = (int64_t)1 << 62;
    P.sweeps = 1;
    P.scratch = base + 3 * total;                          // per train: [cur0 | cur1 | M2 | LQ / Jacobi scratch]
    P.scratch_stride = per_train;
    P.pmax = (int)pmax; P.qmax = (int)qmax;
    P.status = z->d_status;
    P.sweep_stats = z->d_status + batch;
    H.tensors = d_in;
    H.total = total;
    H.index = (int)index - 1;
    H.tol = tol;
    H.work = base;
    H.work_stride = per_train;
    hipLaunchKernelGGL(k_ttv_decomp, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, H);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));                // `tensors` is caller memory: do not keep it in flight
    z->bound = bnd;
    for (int b = 0; b < batch; ++b)
        for (int k = 0; k < d; ++k) z->ot[(size_t)b * d + k] = (k < index - 1) ? -1 : (k == index - 1 ? 0 : 1);     // tt_tools.jl:191-198
    return TTN_OK;
}
int ttn_ttv_decomp(ttn_tt_t z, const double* tensors, int64_t index, double tol) { return ttv_decomp_impl(z, tensors, index, tol, false); }
int ttn_ttv_decomp_dev(ttn_tt_t z, const double* d_tensors, int64_t index, double tol) { return ttv_decomp_impl(z, d_tensors, index, tol, true); }

// ---- to_qtt / to_ttv: split and merge sites (csrc/ttn_resite_kernels.h) ----------------------------------------------------------
// to_qtt(tt, split_dims; threshold)   src/qtt_tools.jl:254-310.  z carries the flattened split lists as its dims; its ranks are written per
// train, a rank above z's capacity is that train's TTN_ST_RANK_OVERFLOW.  Asynchronous.
int ttn_tt_split_sites(ttn_tt_t x, ttn_tt_t z, const int64_t* nsplit, const int64_t* split_dims, double threshold) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_split_sites", {x, z});
    if (!x || !z || !nsplit || !split_dims) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: null argument");
    if (x == z) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: output must not alias the input");
    if (!(threshold >= 0.0)) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: threshold must be >= 0");
    const int dx = x->d, dz = z->d, batch = x->batch;
    if (dx > TTN_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_split_sites: more than 64 input sites");
    int64_t nz = 0;
    for (int i = 0; i < dx; ++i) {
        if (nsplit[i] < 1) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: every site needs at least one factor");
        nz += nsplit[i];
    }
    if (nz != dz) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: sum(nsplit) differs from the number of sites of the output handle");
    for (int i = 0, m = 0; i < dx; ++i) {
        int64_t prod = 1;
        for (int64_t j = 0; j < nsplit[i]; ++j, ++m) {
            if (split_dims[m] < 1) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: factors must be >= 1");
            prod *= split_dims[m];
            if (prod > x->dims[i]) break;
        }
        if (prod != x->dims[i]) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: the product of a site's factors differs from its dimension");
    }
    for (int m = 0; m < dz; ++m)
        if (z->dims[m] != split_dims[m]) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: the output handle's dims differ from the flattened split lists");
    if (z->batch != batch) return fail(TTN_ERR_ARG, "ttn_tt_split_sites: batch sizes differ");
    // worst-case unfoldings and carried remainders: input ranks bounded by x's host bound, new ranks by z's capacity (cf. ttn_ttv_decomp)
    std::vector<int64_t> bnd(dz + 1, 1);
    long long pmax = 1, qmax = 1, m2max = 1, carry = 2;
    bnd[0] = x->bound[0];
    if (z->cap[0] < x->bound[0]) return fail(TTN_ERR_CAPACITY, "ttn_tt_split_sites: destination capacity too small at a kept bond");
    for (int i = 0, zi = 0; i < dx; ++i) {
        const long long rnext = x->bound[i + 1];
        long long rprev = x->bound[i], remaining = x->dims[i];
        if (z->cap[zi + nsplit[i]] < rnext) return fail(TTN_ERR_CAPACITY, "ttn_tt_split_sites: destination capacity too small at a kept bond");
        for (int64_t j = 0; j + 1 < nsplit[i]; ++j, ++zi) {
            const long long s = z->dims[zi], fine = remaining / s, a = rprev * s, bc = fine * rnext;
            pmax = std::max(pmax, std::min(a, bc)); qmax = std::max(qmax, std::max(a, bc));
            if (std::min(a, bc) > 4096)
                return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_split_sites: an unfolding has a short side above 4096 (lower the ranks or the rank capacity of the output)");
            if (a * bc > (1LL << 27)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_split_sites: an unfolding has more than 2^27 entries");
            m2max = std::max(m2max, a * bc);
            rprev = std::min<long long>(std::min(a, bc), z->cap[zi + 1]);
            bnd[zi + 1] = rprev;
            carry = std::max(carry, rprev * bc);
            remaining = fine;
        }
        ++zi;
        bnd[zi] = rnext;
    }
    carry = (carry + 1) & ~1LL; m2max = (m2max + 1) & ~1LL;
    const long long per_scr = QR_NB * qmax + pmax * QR_NB + 2 * pmax * pmax + 4 * pmax + 64;
    const long long per_train = 2 * carry + m2max + per_scr;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * batch);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    SplitArgs H;
    memset(&H, 0, sizeof(H));
    CompressArgs& P = H.C;
    P.tt = z->dev();
    P.max_bond = (int64_t)1 << 62;
    P.sweeps = 1;
    P.scratch = base + 2 * carry + m2max;                  // per train: [cur0 | cur1 | M2 | LQ / Jacobi scratch]
    P.scratch_stride = per_train;
    P.pmax = (int)pmax; P.qmax = (int)qmax;
    P.status = z->d_status;
    P.sweep_stats = z->d_status + batch;
    H.x = x->dev();
    for (int i = 0; i < dx; ++i) H.nsplit[i] = (int)nsplit[i];
    H.threshold = threshold;
    H.work = base;
    H.work_stride = per_train;
    H.carry_len = carry;
    hipLaunchKernelGGL(k_split_sites, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, H);
    HIPCHK(hipGetLastError());
    z->bound = bnd;
    std::fill(z->ot.begin(), z->ot.end(), 0);              // qtt_tools.jl:309
    return TTN_OK;
}

// to_ttv(qtt, merge_numbers)   src/qtt_tools.jl:323-360: group g of z is the product of merge_numbers[g] consecutive cores of x, physical
// indices merged big-endian (the earlier core is the more significant digit).  Asynchronous; no SVD, ranks are the kept bonds of x.
int ttn_tt_merge_sites(ttn_tt_t x, ttn_tt_t z, const int64_t* merge_numbers, int64_t ngroups) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_merge_sites", {x, z});
    if (!x || !z || !merge_numbers) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: null argument");
    if (x == z) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: output must not alias the input");
    const int dx = x->d, batch = x->batch;
    int64_t total = 0;
    for (int64_t g = 0; g < ngroups; ++g) {
        if (merge_numbers[g] < 1) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: every group needs at least one core");
        total += merge_numbers[g];
    }
    if (ngroups < 1 || total != dx) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: sum(merge_numbers) differs from the number of sites of the input handle");
    if (ngroups != z->d) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: the number of groups differs from the number of sites of the output handle");
    std::vector<int> first((size_t)ngroups);
    for (int g = 0, k = 0; g < (int)ngroups; k += (int)merge_numbers[g], ++g) {
        first[g] = k;
        int64_t prod = 1;
        for (int s = 0; s < merge_numbers[g]; ++s) { prod *= x->dims[k + s]; if (prod > z->dims[g]) break; }
        if (prod != z->dims[g]) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: the output handle's dims differ from the products of the merged dims");
    }
    if (z->batch != batch) return fail(TTN_ERR_ARG, "ttn_tt_merge_sites: batch sizes differ");
    std::vector<int64_t> bnd((size_t)ngroups + 1);
    for (int g = 0; g <= (int)ngroups; ++g) {
        bnd[g] = x->bound[g < ngroups ? first[g] : dx];
        if (z->cap[g] < bnd[g]) return fail(TTN_ERR_CAPACITY, "ttn_tt_merge_sites: destination capacity too small");
    }
    // workspace: two buffers per group of >= 3 cores, each as large as its largest intermediate product
    std::vector<long long> woff((size_t)ngroups, 0), whalf((size_t)ngroups, 0);
    long long wtot = 0;
    for (int g = 0; g < (int)ngroups; ++g) {
        const int k0 = first[g], cnt = (int)merge_numbers[g];
        long long n = x->dims[k0], half = 0;
        for (int s = 1; s + 1 < cnt; ++s) { n *= x->dims[k0 + s]; half = std::max(half, n * x->bound[k0] * x->bound[k0 + s + 1]); }
        half = (half + 1) & ~1LL;
        woff[g] = wtot; whalf[g] = half; wtot += 2 * half;
    }
    // grid sizes of every launch, checked before the first one: tiles of step `step` over the groups g0 .. g0 + ng - 1 (by x's rank bounds)
    auto step_tiles = [&](int g0, int ng, int step) {
        long long tiles = 1;
        for (int g = g0; g < g0 + ng; ++g) {
            if (merge_numbers[g] <= step) continue;
            const int k0 = first[g];
            long long nA = 1;
            for (int s = 0; s < step; ++s) nA *= x->dims[k0 + s];
            const long long n2 = x->dims[k0 + step];
            const long long CJ = std::min<long long>(n2, TTN_MERGE_NX), CI = std::min<long long>(nA, TTN_MERGE_NX / CJ);
            tiles = std::max(tiles, ((nA + CI - 1) / CI) * ((n2 + CJ - 1) / CJ) * ((x->bound[k0] + 15) / 16) * ((x->bound[k0 + step + 1] + 15) / 16));
        }
        return tiles;
    };
    if (batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_merge_sites: more than 65535 trains in one handle");
    for (int g = 0; g < (int)ngroups; ++g)
        if (z->dims[g] >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_merge_sites: a merged physical dimension of 2^31 or more");
    for (int g0 = 0; g0 < (int)ngroups; g0 += TTN_MERGE_GROUPS) {
        const int ng = std::min<int>(TTN_MERGE_GROUPS, (int)ngroups - g0);
        int maxcnt = 1;
        for (int g = g0; g < g0 + ng; ++g) maxcnt = std::max(maxcnt, (int)merge_numbers[g]);
        for (int step = 1; step < maxcnt; ++step)
            if (step_tiles(g0, ng, step) >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_merge_sites: more than 2^31 output tiles in one core");
    }
    int rc = scratch_take(sizeof(double) * (size_t)std::max<long long>(2, wtot) * batch);
    if (rc) return rc;
    for (int g0 = 0; g0 < (int)ngroups; g0 += TTN_MERGE_GROUPS) {
        const int ng = std::min<int>(TTN_MERGE_GROUPS, (int)ngroups - g0);
        MergeArgs M;
        memset(&M, 0, sizeof(M));
        M.x = x->dev(); M.z = z->dev(); M.status = z->d_status; M.ngroups = ng; M.g0 = g0;
        M.work = g_scratch.as<double>(); M.work_stride = wtot;
        int maxcnt = 1;
        long long copy_len = 1;
        for (int g = 0; g < ng; ++g) {
            const int k0 = first[g0 + g], cnt = (int)merge_numbers[g0 + g];
            M.k0[g] = k0; M.count[g] = cnt; M.work_off[g] = woff[g0 + g]; M.work_half[g] = whalf[g0 + g];
            maxcnt = std::max(maxcnt, cnt);
            if (cnt == 1) copy_len = std::max<long long>(copy_len, x->dims[k0] * x->bound[k0] * x->bound[k0 + 1]);
        }
        const unsigned cblocks = (unsigned)std::min<long long>((copy_len + TTN_MERGE_TB - 1) / TTN_MERGE_TB, 1024);
        hipLaunchKernelGGL(k_merge_copy, dim3(cblocks, (unsigned)ng, (unsigned)batch), dim3(TTN_MERGE_TB), 0, g_stream, M);
        HIPCHK(hipGetLastError());
        for (int step = 1; step < maxcnt; ++step) {
            M.step = step;
            hipLaunchKernelGGL(k_merge_step, dim3((unsigned)step_tiles(g0, ng, step), (unsigned)ng, (unsigned)batch), dim3(TTN_MERGE_TB), 0, g_stream, M);
            HIPCHK(hipGetLastError());
        }
    }
    z->bound = bnd;
    std::fill(z->ot.begin(), z->ot.end(), 0);              // qtt_tools.jl:359
    return TTN_OK;
}

// ---- train -> dense tensor (csrc/ttn_grid_kernels.h) --------------------------------------------------------------------------------
static long long g_dense_plan[3] = {-1, 0, 0};   // cut m, TM, TN of the last ttn_tt_to_dense / ttn_tto_to_dense (ttn_debug_dense_plan); m < 0: none
static long long g_gather_plan[4] = {0, 0, 0, 0};   // TI, TO, ld, RO of the gather of the last ttn_tto_decomp_dev (ttn_debug_gather_plan); TI == 0: none
// One side's partial products, enqueued step by step: the small steps share single-workgroup launches, a large step gets the grid.
// Returns the buffer (0 / 1) that holds the last step's result.  `dims` / `bound`: the host copies of the view's dimensions and rank bounds.
static int dense_chain(const TTDev& tt, const int64_t* dims, const int64_t* bound, int batch, int side, int k_first, int nsteps, double* buf0,
                       double* buf1, long long buf_stride) {
    DenseChainArgs C;
    C.tt = tt; C.side = side; C.buf[0] = buf0; C.buf[1] = buf1; C.buf_stride = buf_stride;
    long long P = 1;
    int g = 0;
    auto site = [&](int s) { return side == 0 ? k_first + s : k_first - s; };
    auto outputs = [&](int s, long long rows_in) {
        const int k = site(s);
        return rows_in * dims[k] * dense_ld(side == 0 ? bound[k + 1] : bound[k]);
    };
    while (g < nsteps) {
        const long long big = outputs(g, P);
        long long Pg = P * dims[site(g)];
        int cnt = 1;
        if (big <= TTN_DENSE_CHAIN_SMALL)
            while (g + cnt < nsteps && outputs(g + cnt, Pg) <= TTN_DENSE_CHAIN_SMALL) { Pg *= dims[site(g + cnt)]; ++cnt; }
        C.k0 = site(g); C.nsteps = cnt; C.par = g & 1;
        const unsigned blocks = big <= TTN_DENSE_CHAIN_SMALL ? 1u : (unsigned)std::min<long long>((big + TTN_DENSE_TB - 1) / TTN_DENSE_TB, 4096);
        hipLaunchKernelGGL(k_dense_chain, dim3(blocks, (unsigned)batch), dim3(TTN_DENSE_TB), 0, g_stream, C);
        P = Pg;
        g += cnt;
    }
    return (nsteps - 1) & 1;
}

// A digit of the output address: a factor n of site `site`'s dimension with its output stride; `sub` is its stride inside the site's
// own index.  A vector site is one digit (sub = 1); operator site k, seen as a site of dimension n_k^2 with merged index x + n_k y, is
// two: x_k (sub = 1) and y_k (sub = n_k).
struct DenseDigit {
    int site, n;
    long long ostride, sub;
};

// Digits with n > 1 by ascending stride (a digit with n = 1 has none), checked to be a mixed-radix system: a bijection onto [0, total).
static bool mixed_radix_order(const std::vector<int>& n, const std::vector<long long>& stride, std::vector<int>& order) {
    order.clear();
    for (int j = 0; j < (int)n.size(); ++j) if (n[j] > 1) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return stride[a] < stride[b]; });
    long long expect = 1;
    for (int j : order) {
        if (stride[j] != expect) return false;
        expect *= n[j];
    }
    return true;
}

// The body of ttn_tt_to_dense and ttn_tto_to_dense: `tt` is a view of `batch` trains on d sites with host dimensions `dims` (every
// one <= its digits' product), host rank bounds `bound` and end ranks 1; `digits` lists the digits of every site in train order.  The
// callers have checked the sizes (total <= 2^27, every digit's n <= TTN_DENSE_TILE, d <= TTN_MAX_D).
static int dense_export(const char* who, const TTDev& tt, const int64_t* dims, const int64_t* bound, int batch, const std::vector<DenseDigit>& digits,
                        double* d_out) {
    const int d = tt.d;
    long long total = 1;
    for (int k = 0; k < d; ++k) total *= dims[k];
    std::vector<int> order;
    {
        std::vector<int> dn(digits.size());
        std::vector<long long> ds(digits.size());
        for (size_t j = 0; j < digits.size(); ++j) { dn[j] = digits[j].n; ds[j] = digits[j].ostride; }
        if (!mixed_radix_order(dn, ds, order))
            return fail(TTN_ERR_ARG, (std::string(who) + ": the strides are not a mixed-radix system (smallest 1, each next = previous * its n)").c_str());
    }
    // the cut m in 0..d-1 (sites 0..m-1 left, m..d-1 right): both partial products about sqrt(total) wide, the first minimiser.  m = 0
    // happens only when no cut inside the train is better, i.e. for one site (or leading sites of dimension 1): the left side is
    // then empty and L is the 1 x 1 unit.
    int m = 0;
    long long PL = 1;
    {
        long long p = 1, best = -1;
        for (int c = 0; c < d; ++c) {
            const long long wide = std::max(p, total / p);
            if (best < 0 || wide < best) { best = wide; m = c; PL = p; }
            p *= dims[c];
        }
    }
    const long long PR = total / PL;
    // the tile: the lowest-stride digits while their n multiply to at most TTN_DENSE_TILE
    DenseTabArgs TL, TR;
    memset(&TL, 0, sizeof(TL)); memset(&TR, 0, sizeof(TR));
    int TM = 1, TN = 1;
    {
        bool open = true;
        std::vector<long long> rs(d);                        // stride of site k in the row index of L / the column index of R
        { long long s = 1; for (int k = 0; k < m; ++k) { rs[k] = s; s *= dims[k]; } s = 1; for (int k = m; k < d; ++k) { rs[k] = s; s *= dims[k]; } }
        for (int j : order) {
            const DenseDigit& g = digits[j];
            if (open && (long long)TM * TN * g.n <= TTN_DENSE_TILE) { if (g.site < m) TM *= g.n; else TN *= g.n; }
            else open = false;
            DenseTabArgs& T = g.site < m ? TL : TR;
            T.n[T.ns] = g.n; T.stride[T.ns] = g.ostride; T.rstride[T.ns] = rs[g.site] * g.sub; ++T.ns;
        }
    }
    // scratch: [unit | offL | offR | rowL | colR | L ping-pong | R ping-pong]
    long long szL = 4, szR = 4;
    { long long p = 1; for (int k = 0; k < m; ++k) { p *= dims[k]; szL = std::max(szL, p * dense_ld(bound[k + 1])); } }
    { long long p = 1; for (int k = d - 1; k >= m; --k) { p *= dims[k]; szR = std::max(szR, p * dense_ld(bound[k])); } }
    auto pad4 = [](long long v) { return (v + 3) & ~3LL; };
    const long long o_unit = 0, o_offL = 4, o_offR = o_offL + pad4(PL), o_rowL = o_offR + pad4(PR), o_colR = o_rowL + pad4((PL + 1) / 2),
                    o_L = o_colR + pad4((PR + 1) / 2), o_R = o_L + 2 * szL * batch, o_end = o_R + 2 * szR * batch;
    int rc = scratch_take(sizeof(double) * (size_t)o_end);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    if (m == 0) {
        static const double unit[4] = {1.0, 0.0, 0.0, 0.0};
        HIPCHK(hipMemcpyAsync(base + o_unit, unit, sizeof(unit), hipMemcpyHostToDevice, g_stream));
    }
    TL.count = PL; TL.off = reinterpret_cast<long long*>(base + o_offL); TL.idx = reinterpret_cast<int*>(base + o_rowL);
    TR.count = PR; TR.off = reinterpret_cast<long long*>(base + o_offR); TR.idx = reinterpret_cast<int*>(base + o_colR);
    for (DenseTabArgs* T : {&TL, &TR}) {
        const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((T->count + TTN_DENSE_TB - 1) / TTN_DENSE_TB, 1024));
        hipLaunchKernelGGL(k_dense_tables, dim3(blocks), dim3(TTN_DENSE_TB), 0, g_stream, *T);
    }
    double* Lb = base + o_L;
    double* Rb = base + o_R;
    DenseArgs A;
    memset(&A, 0, sizeof(A));
    if (m > 0) { const int w = dense_chain(tt, dims, bound, batch, 0, 0, m, Lb, Lb + szL * batch, szL); A.L = w ? Lb + szL * batch : Lb; A.strideL = szL; }
    else { A.L = base + o_unit; A.strideL = 0; }
    { const int w = dense_chain(tt, dims, bound, batch, 1, d - 1, d - m, Rb, Rb + szR * batch, szR); A.R = w ? Rb + szR * batch : Rb; A.strideR = szR; }
    A.rks = tt.rks; A.d = d; A.m = m;
    A.offL = TL.off; A.offR = TR.off; A.rowL = TL.idx; A.colR = TR.idx;
    A.tilesL = PL / TM; A.TM = TM; A.TN = TN; A.total = total; A.out = d_out;
    g_dense_plan[0] = m; g_dense_plan[1] = TM; g_dense_plan[2] = TN;
    const long long seg = (long long)TM * TN;
    A.vec2 = (seg % 2 == 0 && (total % 2 == 0 || batch == 1) && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_dense_product, dim3((unsigned)(total / seg), (unsigned)batch), dim3(TTN_DENSE_TB), 0, g_stream, A);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_tt_to_dense(ttn_tt_t x, const int64_t* strides, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_to_dense", {x});
    if (!x || !d_out) return fail(TTN_ERR_ARG, "null argument");
    const int d = x->d;
    if (d > TTN_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_to_dense: more than 64 sites");
    if (x->bound[0] != 1 || x->bound[d] != 1) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_to_dense: the end ranks must be 1");
    long long total = 1;
    for (int k = 0; k < d; ++k) {
        total *= x->dims[k];
        if (total > (1LL << 27)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_to_dense: more than 2^27 entries per train");
        // a tile is made of whole digits: a dimension above the tile size would leave one workgroup per output element
        if (x->dims[k] > TTN_DENSE_TILE) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_to_dense: a physical dimension above 4096");
    }
    // output strides: Julia column-major unless given; one digit per site
    std::vector<DenseDigit> digits(d);
    { long long s = 1; for (int k = 0; k < d; ++k) { digits[k] = DenseDigit{k, (int)x->dims[k], strides ? (long long)strides[k] : s, 1}; s *= x->dims[k]; } }
    return dense_export("ttn_tt_to_dense", x->dev(), x->dims.data(), x->bound.data(), x->batch, digits, d_out);
}

// ---- operator <-> dense array (include/ttn_dense.h) -----------------------------------------------------------------------------------
// The two stride tables of an operator's dense array, or the reference's [x_1..x_d, y_1..y_d] column-major array when both are null.
static void operator_strides(int d, const int64_t* dims, const int64_t* xstrides, const int64_t* ystrides, std::vector<long long>& xs, std::vector<long long>& ys) {
    xs.resize(d); ys.resize(d);
    long long N = 1;
    for (int k = 0; k < d; ++k) N *= dims[k];
    long long s = 1;
    for (int k = 0; k < d; ++k) {
        xs[k] = xstrides ? (long long)xstrides[k] : s;
        ys[k] = ystrides ? (long long)ystrides[k] : N * s;
        s *= dims[k];
    }
}

int ttn_debug_dense_plan(int64_t* out3) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!out3 || g_dense_plan[0] < 0) return fail(TTN_ERR_ARG, "ttn_debug_dense_plan: no ttn_tt_to_dense / ttn_tto_to_dense launch yet");
    for (int i = 0; i < 3; ++i) out3[i] = g_dense_plan[i];
    return TTN_OK;
}

int ttn_debug_gather_plan(int64_t* out4) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!out4 || g_gather_plan[0] == 0) return fail(TTN_ERR_ARG, "ttn_debug_gather_plan: no ttn_tto_decomp_dev launch yet");
    for (int i = 0; i < 4; ++i) out4[i] = g_gather_plan[i];
    return TTN_OK;
}

int ttn_tto_to_dense(ttn_tto_t A, const int64_t* xstrides, const int64_t* ystrides, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_to_dense", {}, {A});
    if (!A || !d_out) return fail(TTN_ERR_ARG, "ttn_tto_to_dense: null argument");
    if (int rb = single_op(A, "ttn_tto_to_dense")) return rb;
    if ((xstrides == nullptr) != (ystrides == nullptr)) return fail(TTN_ERR_ARG, "ttn_tto_to_dense: xstrides and ystrides must both be given or both be null");
    const int d = A->d;
    if (d > TTN_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_to_dense: more than 64 sites");
    if (A->rks[0] != 1 || A->rks[d] != 1) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_to_dense: the end ranks must be 1");
    std::vector<int64_t> dims2(d);
    long long total = 1;
    for (int k = 0; k < d; ++k) {
        // the limit of a tile holds per digit: n_k^2 may exceed it, the tile then splits the site between x_k and y_k
        if (A->dims[k] > TTN_DENSE_TILE) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_to_dense: a physical dimension above 4096");
        dims2[k] = A->dims[k] * A->dims[k];
        total *= dims2[k];
        if (total > (1LL << 27)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_to_dense: more than 2^27 entries");
    }
    std::vector<long long> xs, ys;
    operator_strides(d, A->dims.data(), xstrides, ystrides, xs, ys);
    std::vector<DenseDigit> digits;
    for (int k = 0; k < d; ++k) {
        digits.push_back(DenseDigit{k, (int)A->dims[k], xs[k], 1});
        digits.push_back(DenseDigit{k, (int)A->dims[k], ys[k], (long long)A->dims[k]});
    }
    return dense_export("ttn_tto_to_dense", A->vdev(), dims2.data(), A->rks.data(), 1, digits, d_out);
}

int ttn_qtt_grid_points(int64_t n_dims, int64_t bits, int interleaved, double a, double b, int64_t first, int64_t count, double* d_X) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!d_X) return fail(TTN_ERR_ARG, "null argument");
    if (n_dims < 1 || bits < 1 || bits > 52 || n_dims * bits > 62) return fail(TTN_ERR_ARG, "ttn_qtt_grid_points: need n_dims >= 1, 1 <= bits <= 52, n_dims * bits <= 62");
    if (first < 0 || count < 0 || count > ((int64_t)1 << (n_dims * bits)) - first) return fail(TTN_ERR_ARG, "ttn_qtt_grid_points: first .. first + count - 1 leaves the tensor");
    if (count == 0) return TTN_OK;
    const double h = (b - a) / (double)(((int64_t)1 << bits) - 1);
    const unsigned blocks = (unsigned)std::min<long long>((count + TTN_DENSE_TB - 1) / TTN_DENSE_TB, 4096);
    hipLaunchKernelGGL(k_qtt_grid_points, dim3(blocks), dim3(TTN_DENSE_TB), 0, g_stream, (int)n_dims, (int)bits, interleaved ? 1 : 0, a, h,
                       (long long)first, (long long)count, d_X);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

// ---- als_linsolve ------------------------------------------------------------------------------------------------
#define TTN_DENSE_LOCAL_MAX_ALS 2048
static DevBuf g_lu_flag;          // singular-pivot word of the grid form of als_linsolve
// The grid form of als_linsolve (csrc/ttn_als_grid.h): for every train in turn the half sweeps of src/solvers/als.jl:199-219 walked on
// the host — per site the assembly of K (grid), the blocked LU with partial pivoting panel by panel (panel: one workgroup; row
// interchanges + U12: grid; trailing MFMA update: grid), the back substitution, then the core move and environment update (phase 2 / 3
// of k_als_linsolve, one workgroup).  Everything is enqueued on the library stream; one flag word carries a singular pivot column.
// The blocked LU of the grid form, panel by panel, on K (N x N column-major, destroyed) and rhs (the solution on return); piv: N
// ints, flag: the singular-pivot word (every stage returns at once while it is set).  Shared by als_grid_path and the kernel
// unit-test hook ttn_selftest_lu_solve.  Enqueues only.
static void lu_grid_solve(double* K, double* Pb, int N, int* piv, int* d_flag) {
    for (int k0 = 0; k0 < N; k0 += LU_NB) {
        const int w = std::min(LU_NB, N - k0);
        hipLaunchKernelGGL(k_lu_panel, dim3(1), dim3(TTN_WG), LU_PANEL_LDS_BYTES, g_stream, K, N, k0, w, piv, d_flag);
        hipLaunchKernelGGL(k_lu_rows, dim3((N + 1 + 255) / 256), dim3(256), 0, g_stream, K, Pb, N, k0, w, (const int*)piv, (const int*)d_flag);
        const int m = N - k0 - w;
        if (m > 0) {
            const int nt = (m + LU_TILE - 1) / LU_TILE;
            hipLaunchKernelGGL(k_lu_trail, dim3(nt, nt), dim3(TTN_WG), sizeof(double) * GEMM_LDS_TOTAL, g_stream, K, Pb, N, k0, w, (const int*)d_flag);
        }
    }
    for (int kb = ((N - 1) / 32) * 32; kb >= 0; kb -= 32) {
        const int wb = std::min(32, N - kb);
        hipLaunchKernelGGL(k_lu_back_tri, dim3(1), dim3(64), 0, g_stream, (const double*)K, Pb, N, kb, wb, (const int*)d_flag);
        if (kb > 0) hipLaunchKernelGGL(k_lu_back_rows, dim3((kb + 255) / 256), dim3(256), 0, g_stream, (const double*)K, Pb, N, kb, wb, (const int*)d_flag);
    }
}

static int als_grid_path(AlsArgs P, const std::vector<long long>& off, const std::vector<int64_t>& r, ttn_tto_t A, ttn_tt_t b, ttn_tt_t x, int sweep_count) {
    const int d = x->d, batch = x->batch;
    double* scr = P.scratch;
    double* K = scr + P.offK;
    double* Pb = scr + P.offPb;
    int* piv = reinterpret_cast<int*>(scr + P.offPiv);
    { const int rc = g_lu_flag.ensure(sizeof(int)); if (rc) return rc; }
    int* d_flag = g_lu_flag.as<int>();
    const std::vector<int64_t>& R = A->rks;
    // the right-hand sides of a batch may differ in ranks: phases 1 - 3 lay Gb / Hb out with the train's own, so must the assembly
    std::vector<long long> h_brks((size_t)batch * (d + 1));
    HIPCHK(hipMemcpyAsync(h_brks.data(), b->d_rks, sizeof(long long) * h_brks.size(), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    auto solve_site = [&](int i, int tb) -> int {
        const int n = (int)x->dims[i], rl = (int)r[i], rr = (int)r[i + 1];
        const int nr = n * rl, N = nr * rr;
        AlsAssembleArgs Q;
        Q.G = scr + off[i]; Q.Gb = scr + off[d + i]; Q.H = scr + off[2 * d + i]; Q.Hb = scr + off[3 * d + i];
        Q.K = K; Q.Pb = Pb; Q.nr = nr; Q.rr = rr; Q.Rr = (int)R[i + 1]; Q.br = (int)h_brks[(size_t)tb * (d + 1) + i + 1];
        hipLaunchKernelGGL(k_als_assemble, dim3((N + ALS_ASM_ROWS - 1) / ALS_ASM_ROWS, (N + ALS_ASM_COLS - 1) / ALS_ASM_COLS), dim3(ALS_ASM_ROWS), 0, g_stream, Q);
        lu_grid_solve(K, Pb, N, piv, d_flag);
        HIPCHK(hipGetLastError());
        return TTN_OK;
    };
    auto phase = [&](int ph, int site, int tb) -> int {
        AlsArgs Q = P;
        Q.phase = ph; Q.site = site; Q.train0 = tb;
        hipLaunchKernelGGL(k_als_linsolve, dim3(1), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Q);
        HIPCHK(hipGetLastError());
        return TTN_OK;
    };
    for (int tb = 0; tb < batch; ++tb) {
        HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), g_stream));
        int rc = phase(1, 0, tb);
        if (rc) return rc;
        int nsweeps = 0;
        while (nsweeps < sweep_count) {
            ++nsweeps;
            for (int i = 0; i < d - 1; ++i) { if ((rc = solve_site(i, tb))) return rc; if ((rc = phase(2, i, tb))) return rc; }
            if (nsweeps == sweep_count) break;
            ++nsweeps;
            for (int i = d - 1; i >= 1; --i) { if ((rc = solve_site(i, tb))) return rc; if ((rc = phase(3, i, tb))) return rc; }
        }
        int h_flag = 0;
        HIPCHK(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        if (h_flag) {                                   // LAPACK's SingularException: recorded on the handle like the one-workgroup form does
            const int singular = TTN_ST_SINGULAR;
            HIPCHK(hipMemcpyAsync(x->d_status + tb, &singular, sizeof(int), hipMemcpyHostToDevice, g_stream));
            HIPCHK(hipStreamSynchronize(g_stream));
        }
    }
    return TTN_OK;
}

int ttn_als_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, int64_t sweep_count) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_als_linsolve", {b, x0, x}, {A});
    if (!A || !b || !x0 || !x) return fail(TTN_ERR_ARG, "null handle");
    if (int rb = single_op(A, "ttn_als_linsolve")) return rb;
    if (sweep_count < 1) return fail(TTN_ERR_SWEEPS, "sweep_count must be >= 1");
    if (!same_dims(A->dims, b->dims) || !same_dims(b->dims, x0->dims) || !same_dims(x0->dims, x->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (b->batch != x0->batch || x->batch != x0->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    const int d = x0->d;
    if (d < 2) return fail(TTN_ERR_UNSUPPORTED, "ttn_als_linsolve: needs at least two sites");
    // the solution keeps the ranks of the start train (als.jl:177); they must survive orthogonalize (als.jl:174) and allow
    // the thin QRs of the core moves
    std::vector<int64_t> capped(d + 1);
    ttn_r_and_d_to_rks(d, x0->dims.data(), d + 1, x0->bound.data(), 1024, capped.data());
    const std::vector<int64_t> r(x0->bound);
    for (int k = 0; k <= d; ++k) if (capped[k] != r[k]) return fail(TTN_ERR_UNSUPPORTED, "ttn_als_linsolve: the start ranks exceed what orthogonalize keeps");
    for (int i = 0; i < d; ++i)
        if (x0->dims[i] * r[i] < r[i + 1] || x0->dims[i] * r[i + 1] < r[i]) return fail(TTN_ERR_UNSUPPORTED, "ttn_als_linsolve: a core is too flat for the QR core moves");
    int rc = ttn_orthogonalize(x0, 1, x);
    if (rc) return rc;
    const std::vector<int64_t>& R = A->rks;
    const std::vector<int64_t>& rb = b->bound;
    std::vector<long long> off(4 * d);
    long long cur = 0, Nmax = 1, mmax = 1, rmax = 1, t1 = 1, t2 = 1;
    for (int i = 0; i < d; ++i) {
        const long long n = x0->dims[i], rl = r[i], rr = r[i + 1], Rl = R[i], Rr = R[i + 1], bl = rb[i], br = rb[i + 1];
        off[i] = cur; cur += n * rl * n * rl * Rr;
        off[d + i] = cur; cur += n * rl * br;
        off[2 * d + i] = cur; cur += Rr * rr * rr;
        off[3 * d + i] = cur; cur += rr * br;
        Nmax = std::max(Nmax, n * rl * rr);
        mmax = std::max(mmax, std::max(n * rl, n * rr));
        rmax = std::max(rmax, std::max(rl, rr));
        t1 = std::max(t1, std::max(std::max(Rr * rr * n * rl, n * rl * rr * std::max(Rl, Rr)), std::max(rr * n * bl, std::max(rr * br, rl * br))));
        t2 = std::max(t2, std::max(n * rr * Rl * rl, rr * rr * Rr));
    }
    // Local systems above 2048 unknowns (ranks above 32 for n = 2 — BASELINE config C5 names ranks up to 128: 32 768 unknowns, an 8.6 GB
    // matrix): the GRID form — assembly and LU on the whole chip, the host walks the half sweeps (als_grid_path below).
    const bool grid_path = Nmax > TTN_DENSE_LOCAL_MAX_ALS || (getenv("TTN_ALS_GRID") && atoi(getenv("TTN_ALS_GRID")) != 0);
    if (Nmax > 65536) return fail(TTN_ERR_UNSUPPORTED, "ttn_als_linsolve: local systems above 65 536 unknowns are not supported");
    AlsArgs P;
    memset(&P, 0, sizeof(P));
    P.offK = cur; cur += Nmax * Nmax;
    P.offPb = cur; cur += Nmax;
    P.offPiv = cur; cur += Nmax / 2 + 8;               // Nmax ints
    P.offT1 = cur; cur += t1;
    P.offT2 = cur; cur += t2;
    P.offTm = cur; cur += mmax * rmax;
    P.offQb = cur; cur += mmax * rmax;
    P.offRb = cur; cur += rmax * rmax;
    P.offVb = cur; cur += QR_NB * mmax;
    P.offWb = cur; cur += QR_NB * mmax;
    P.offTst = cur; cur += ((rmax + QR_NB - 1) / QR_NB) * QR_NB * QR_NB + 64;
    const long long per_train = cur;
    const int batch = x->batch;
    const int nslots = grid_path ? 1 : batch;          // the grid form works on one train at a time (K alone can be gigabytes)
    rc = scratch_take(sizeof(double) * (size_t)per_train * nslots + sizeof(long long) * (size_t)(5 * d + 1) + 64);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * batch);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    long long* d_tab = (long long*)(base + (size_t)per_train * nslots);
    std::vector<long long> h_off(off);
    h_off.insert(h_off.end(), r.begin(), r.end());
    HIPCHK(hipMemcpyAsync(d_tab, h_off.data(), sizeof(long long) * h_off.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));            // h_off is a local
    P.A = A->dev(); P.b = b->dev(); P.x = x->dev();
    P.sweep_count = (int)sweep_count;
    P.scratch = base; P.scratch_stride = per_train;
    P.off = d_tab;
    P.rfix = d_tab + 4 * d;
    P.mmax = (int)mmax; P.rmax = (int)rmax;
    P.status = x->d_status;
    if (grid_path) {
        rc = als_grid_path(P, off, r, A, b, x, (int)sweep_count);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_als_linsolve, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, P);
        HIPCHK(hipGetLastError());
    }
    // orthogonality flags as the core moves leave them (als.jl:128-134, :112-118)
    for (int bb = 0; bb < batch; ++bb) {
        int64_t* ot = &x->ot[(size_t)bb * d];
        int64_t done = 0;
        while (done < sweep_count) {
            ++done;
            for (int i = 0; i + 1 < d; ++i) { ot[i] = -1; ot[i + 1] = 0; }
            if (done == sweep_count) break;
            ++done;
            for (int i = d - 1; i >= 1; --i) { ot[i] = 1; ot[i - 1] = 0; }
        }
    }
    return TTN_OK;
}

// ---- the two-site solvers (mals_linsolve / dmrg_linsolve, mals_eigsolve / dmrg_eigsolve) ---------------------------------------
// The sweep plan of a stage schedule: plan[s] = the rank cap of full sweep s (rmax_schedule null: 1).  The reference's while-loops
// (dmrg.jl:421-426, :523-528, mals.jl:372-378) only terminate for positive, strictly increasing stage ends.  Messages start with `who`;
// more than TTN_DMRG_MAX_SWEEPS sweeps fail with `too_many`.
static int sweep_plan(const char* who, int too_many, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                      std::vector<int64_t>& plan) {
    auto bad = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
    if (n_stages < 1 || !sweep_schedule) return bad(TTN_ERR_ARG, "empty schedule");
    for (int64_t j = 0; j < n_stages; ++j) {
        if (sweep_schedule[j] < 1 || (j && sweep_schedule[j] <= sweep_schedule[j - 1])) return bad(TTN_ERR_ARG, "sweep_schedule must be positive and strictly increasing");
        if (rmax_schedule && rmax_schedule[j] < 1) return bad(TTN_ERR_ARG, "bad rmax_schedule");
    }
    if (sweep_schedule[n_stages - 1] - 1 > TTN_DMRG_MAX_SWEEPS) return bad(too_many, "more than 32 sweeps in one call");
    plan.clear();
    int64_t n = 0, j = 0;
    for (;;) {
        ++n;
        if (n == sweep_schedule[j]) { if (++j >= n_stages) break; }
        plan.push_back(rmax_schedule ? rmax_schedule[j] : 1);
    }
    return TTN_OK;
}

// Workspace of one train.  Slots per site i: G_i (off[i]) and, for the window (i, i+1), H_i (off[2d + i]); with a right-hand side
// also its projections Gb_i (off[d + i]) and Hb_i (off[3d + i]).  `cur` is the end of what is laid out so far, in doubles.
struct TwoSiteLayout {
    std::vector<long long> off;
    long long cur = 0, Nmax = 1, mmax = 1, t1 = 1, t2 = 1, Rzmax = 1, pmax = 1, qmax = 1;
};

// c: capacity ranks of the result, R: operator ranks, rb: bounds of the right-hand side (null: eigensolver, no rhs slots / terms)
static TwoSiteLayout two_site_slots(const std::vector<int64_t>& dims, const std::vector<int64_t>& c, const std::vector<int64_t>& R,
                                    const std::vector<int64_t>* rb) {
    const int d = (int)dims.size();
    auto mx = [](long long a_, long long b_) { return a_ > b_ ? a_ : b_; };
    TwoSiteLayout L;
    L.off.assign(4 * d, 0);
    long long& cur = L.cur;
    for (int i = 0; i < d; ++i) {
        const long long n = dims[i];
        L.off[i] = cur; cur += n * c[i] * n * c[i] * R[i + 1];
        if (rb) { L.off[d + i] = cur; cur += n * c[i] * (*rb)[i + 1]; }
        L.mmax = mx(L.mmax, mx(n * c[i], n * c[i + 1]));
        L.t1 = mx(L.t1, n * c[i] * c[i + 1] * mx(R[i], R[i + 1]));
        if (rb) L.t1 = mx(L.t1, mx(c[i + 1] * (*rb)[i + 1], c[i] * (*rb)[i + 1]));
        L.t2 = mx(L.t2, c[i + 1] * c[i + 1] * R[i + 1]);
        L.Rzmax = mx(L.Rzmax, R[i + 1]);
        if (i + 1 < d) {
            const long long n2 = dims[i + 1];
            L.off[2 * d + i] = cur; cur += R[i + 1] * n2 * n2 * c[i + 2] * c[i + 2];
            if (rb) { L.off[3 * d + i] = cur; cur += (*rb)[i + 1] * n2 * c[i + 2]; }
            L.Nmax = mx(L.Nmax, n * c[i] * n2 * c[i + 2]);
            L.t1 = mx(L.t1, R[i + 1] * n2 * c[i + 2] * c[i + 1]);
            if (rb) L.t1 = mx(L.t1, (*rb)[i + 1] * c[i + 1]);
            L.t2 = mx(L.t2, R[i + 1] * c[i + 1] * c[i + 1]);
        }
    }
    L.pmax = std::min<long long>(L.mmax, 256);
    L.qmax = L.mmax;
    return L;
}

// the blocks of the SVD core moves, after each solver's local-solve blocks
static void two_site_core_move_blocks(TwoSiteLayout& L, MalsArgs& Q) {
    long long& cur = L.cur;
    Q.L.offT1 = cur; cur += L.t1;
    Q.L.offT2 = cur; cur += L.t2;
    Q.L.offVb = cur; cur += QR_NB * L.qmax;
    Q.L.offWb = cur; cur += QR_NB * L.qmax;
    Q.offM2 = cur; cur += L.Nmax;
    Q.offXg = cur; cur += L.pmax * L.pmax;
    Q.offUs = cur; cur += L.pmax * L.pmax;
    Q.offSig = cur; cur += 4 * L.pmax + 64;
}

static size_t two_site_bytes(const TwoSiteLayout& L, int batch) {
    return sizeof(double) * (size_t)L.cur * batch + sizeof(long long) * L.off.size() + 64;
}

// Scratch for the batch, the slot table uploaded behind it, and the kernel arguments both solvers share.  b is the right-hand side
// (the eigensolvers pass x); rmax caps the last stage.
static int two_site_prelude(MalsArgs& Q, const TwoSiteLayout& L, ttn_tto_t A, ttn_tt_t b, ttn_tt_t x, double tol, int64_t rmax, int mode,
                            const std::vector<int64_t>& plan) {
    const int batch = x->batch;
    int rc = scratch_take(two_site_bytes(L, batch));
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * batch);
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    long long* d_tab = (long long*)(base + (size_t)L.cur * batch);
    HIPCHK(hipMemcpyAsync(d_tab, L.off.data(), sizeof(long long) * L.off.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));            // L.off is the caller's
    AlsArgs& P = Q.L;
    P.A = A->dev(); P.b = b->dev(); P.x = x->dev();
    P.scratch = base; P.scratch_stride = L.cur;
    P.off = d_tab;
    P.status = x->d_status;
    Q.C.status = x->d_status;
    Q.C.sweep_stats = x->d_status + batch;
    Q.C.pmax = (int)L.pmax; Q.C.qmax = (int)L.qmax;
    Q.tol = tol;
    Q.rmax = (int)std::min<int64_t>(rmax, 1 << 30);
    Q.rmax_final = Q.rmax;
    Q.pmax = (int)L.pmax; Q.qmax = (int)L.qmax;
    Q.mode = mode;
    Q.nsweeps = (int)plan.size();
    for (size_t s_ = 0; s_ < plan.size(); ++s_) Q.rmax_sweep[s_] = (int)std::min<int64_t>(plan[s_], 1 << 30);
    return TTN_OK;
}

// What the solve leaves on the host side of x: ranks bounded by the largest cap of the plan (and rtop), and the orthogonality flags
// (mals: after the backward half sweep, right-orthogonal cores, mals.jl:116-117; dmrg: left_core_move!, dmrg.jl:222-223, :440, :566)
static void two_site_epilogue(ttn_tt_t x, int mode, const std::vector<int64_t>& plan, int64_t rtop) {
    const int d = x->d;
    for (int64_t r : plan) rtop = std::max(rtop, r);
    for (int m = 1; m < d; ++m) x->bound[m] = std::min<int64_t>(x->cap[m], rtop);
    x->bound[0] = 1; x->bound[d] = 1;
    for (int bb = 0; bb < x->batch; ++bb)
        for (int k = 0; k < d; ++k) x->ot[(size_t)bb * d + k] = (k == 0) ? 0 : (mode == 0 ? 1 : -1);
}

// ---- mals_linsolve / dmrg_linsolve --------------------------------------------------------------------------------
// mode 0 = mals_linsolve, mode 1 = dmrg_linsolve (N = 2) with `plan` = the rank cap of every full sweep
// Local solver of the two-site systems (dmrg.jl:92-97): conjugate gradients on the matrix-free operator if `it_solver` or the system
// has more than `itslv_thresh` unknowns, dense LU otherwise.  The dense path holds K in memory and is limited to TTN_DENSE_LOCAL_MAX
// unknowns; larger systems always take the matrix-free path.
#define TTN_DENSE_LOCAL_MAX 2048
#define TTN_KRYLOVDIM_DEFAULT 30       // KrylovKit.KrylovDefaults.krylovdim
struct LocalSolver { int it_solver = 0; int64_t itslv_thresh = TTN_DENSE_LOCAL_MAX; int64_t maxiter = 200; double tol = 1.0e-8; };
static DevBuf g_cg_iters;         // [batch] CG iterations of the last two-site linear solve
static std::vector<int> g_cg_iters_host;       // total CG iterations per train of the last two-site solve (ttn_dmrg_cg_iterations)

static int two_site_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t rmax, int mode, const std::vector<int64_t>& plan,
                             const LocalSolver& ls = LocalSolver()) {
    NEED_INIT();
    F64_ONLY("two-site linear solver", {b, x0, x}, {A});
    if (!A || !b || !x0 || !x) return fail(TTN_ERR_ARG, "null handle");
    if (tol < 0.0 || rmax < 1) return fail(TTN_ERR_ARG, "bad tol / rmax");
    if (!same_dims(A->dims, b->dims) || !same_dims(b->dims, x0->dims) || !same_dims(x0->dims, x->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (b->batch != x0->batch || x->batch != x0->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    const int d = x0->d;
    if (d < 2) return fail(TTN_ERR_UNSUPPORTED, "ttn_mals_linsolve: needs at least two sites");
    int rc = ttn_orthogonalize(x0, 1, x);                  // mals.jl:252 (checks x's capacity against the start ranks)
    if (rc) return rc;
    TwoSiteLayout L = two_site_slots(x0->dims, x->cap, A->rks, &b->bound);
    const long long Nmax = L.Nmax;
    // mals_linsolve has no iterative branch in the reference (Hermitian(K) \ b, mals.jl:148-157): dense only
    const long long dense_max = ls.it_solver ? 0 : std::min<long long>(TTN_DENSE_LOCAL_MAX, mode == 1 ? ls.itslv_thresh : TTN_DENSE_LOCAL_MAX);
    const bool need_cg = mode == 1 && (ls.it_solver || Nmax > dense_max);
    if (!need_cg && Nmax > TTN_DENSE_LOCAL_MAX) return fail(TTN_ERR_UNSUPPORTED, "ttn_mals_linsolve: two-site systems above 2048 unknowns (n_i cap_i n_{i+1} cap_{i+2}) are not supported; lower the capacity of x");
    if (L.mmax > 256) return fail(TTN_ERR_UNSUPPORTED, "two-site solvers: n_i * capacity above 256 (ranks above 128 for n = 2) is not supported by the SVD core moves");
    if (ls.maxiter < 1 || !(ls.tol >= 0.0)) return fail(TTN_ERR_ARG, "dmrg_linsolve: bad linsolv_maxiter / linsolv_tol");
    const long long Rzmax = std::max<long long>(L.Rzmax, A->rks[0]);
    MalsArgs Q;
    memset(&Q, 0, sizeof(Q));
    AlsArgs& P = Q.L;
    long long& cur = L.cur;
    const long long Kdim = std::min<long long>(Nmax, dense_max);
    P.offK = cur; cur += Kdim * Kdim;
    if (need_cg) { Q.offCg = cur; Q.cg_nmax = Nmax; cur += (4 + Rzmax) * Nmax; }
    Q.cg_all = ls.it_solver ? 1 : 0;
    Q.cg_above = (int)std::min<long long>(dense_max, (1LL << 30));
    // KrylovKit's linsolve selector builds CG(maxiter = krylovdim * maxiter) for isposdef problems, krylovdim = KrylovDefaults' 30
    // (the convention src/solvers/euler.jl:29 spells out; the call at src/solvers/dmrg.jl:170 passes maxiter = linsolv_maxiter only)
    Q.cg_maxiter = (int)std::min<int64_t>(TTN_KRYLOVDIM_DEFAULT * ls.maxiter, 1 << 30);
    Q.cg_tol = ls.tol;
    P.offPb = cur; cur += Nmax;
    P.offPiv = cur; cur += Nmax / 2 + 8;
    two_site_core_move_blocks(L, Q);
    const int batch = x->batch;
    rc = two_site_prelude(Q, L, A, b, x, tol, rmax, mode, plan);
    if (rc) return rc;
    if (need_cg) {
        rc = g_cg_iters.ensure(sizeof(int) * batch);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(g_cg_iters.p, 0, sizeof(int) * batch, g_stream));
        Q.cg_iters = g_cg_iters.as<int>();
    }
    hipLaunchKernelGGL(k_mals_linsolve, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Q);
    HIPCHK(hipGetLastError());
    g_cg_iters_host.assign(batch, 0);
    if (need_cg) {
        HIPCHK(hipMemcpyAsync(g_cg_iters_host.data(), g_cg_iters.p, sizeof(int) * batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    two_site_epilogue(x, mode, plan, rmax);
    return TTN_OK;
}

int ttn_mals_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t rmax) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_mals_linsolve")) return rb;
    return two_site_linsolve(A, b, x0, x, tol, rmax, 0, {});
}

static int dmrg_linsolve_impl(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                              const int64_t* rmax_schedule, const LocalSolver& ls) {
    F64_ONLY("ttn_dmrg_linsolve", {b, x0, x}, {A});
    if (!rmax_schedule) return fail(TTN_ERR_ARG, "dmrg_linsolve: empty schedule");
    std::vector<int64_t> plan;
    const int rc = sweep_plan("dmrg_linsolve", TTN_ERR_UNSUPPORTED, n_stages, sweep_schedule, rmax_schedule, plan);
    if (rc) return rc;
    return two_site_linsolve(A, b, x0, x, tol, rmax_schedule[n_stages - 1], 1, plan, ls);
}

int ttn_dmrg_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                      const int64_t* rmax_schedule) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_dmrg_linsolve")) return rb;
    LocalSolver ls;                      // dense LU up to TTN_DENSE_LOCAL_MAX unknowns, matrix-free CG (tol 1e-8) above
    ls.tol = std::max(std::sqrt(std::max(tol, 0.0)), 1.0e-8);       // the reference's default linsolv_tol (dmrg.jl:394)
    return dmrg_linsolve_impl(A, b, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, ls);
}

int ttn_dmrg_linsolve_it(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                         const int64_t* rmax_schedule, int it_solver, int64_t linsolv_maxiter, double linsolv_tol, int64_t itslv_thresh) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_dmrg_linsolve_it")) return rb;
    if (itslv_thresh < 0) return fail(TTN_ERR_ARG, "dmrg_linsolve: bad itslv_thresh");
    LocalSolver ls;
    ls.it_solver = it_solver ? 1 : 0; ls.itslv_thresh = itslv_thresh; ls.maxiter = linsolv_maxiter; ls.tol = linsolv_tol;
    return dmrg_linsolve_impl(A, b, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, ls);
}

int ttn_dmrg_cg_iterations(int64_t batch, int64_t* iters) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!iters || batch < 0 || (size_t)batch > g_cg_iters_host.size()) return fail(TTN_ERR_ARG, "ttn_dmrg_cg_iterations: no two-site solve of that batch size has run");
    for (int64_t t = 0; t < batch; ++t) iters[t] = g_cg_iters_host[(size_t)t];
    return TTN_OK;
}

// ---- dmrg_eigsolve / mals_eigsolve (csrc/ttn_eigsolve_kernels.h) ---------------------------------------------------------------
// Both walk full sweeps of the same plan as dmrg_linsolve (sweep_plan): DMRG windows 0..d-3 forward, d-2..1 backward, then the closing
// solve at window 0 (one history entry more); MALS windows 0..d-2 forward, d-2..0 backward (mals.jl:393-418, sweep s capped at plan[s]).
static DevBuf g_hist_E, g_hist_r; // [batch][hist_len] energy / rank history of the last two-site eigensolve
static DevBuf g_lz_iters, g_lz_res;   // [batch] Lanczos statistics of the last two-site eigensolve
static DevBuf g_eig_ortho;        // [3][batch][n_ortho] doubles of the last penalised eigensolve: weights, 1 / ||phi_j||, overlaps
static std::vector<int> g_lz_iters_host;       // Lanczos operator applications per train of the last eigensolve (ttn_eigsolve_stats)
static std::vector<double> g_lz_res_host;      // largest final Lanczos residual per train of the last eigensolve

// mode 0 MALS, 1 DMRG (N = 2), 2 ALS (als_eigsolve / als_gen_eigsolv: 2 (d - 1) micro-steps per full sweep, like MALS)
static int64_t eig_hist_len(int mode, int64_t d, int64_t nsweeps) { return mode == 1 ? 2 * (d - 2) * nsweeps + 1 : 2 * (d - 1) * nsweeps; }

int ttn_eigsolve_history_len(int mode, int64_t d, int64_t n_stages, const int64_t* sweep_schedule, int64_t* len) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!len || mode < 0 || mode > 2 || d < 2) return fail(TTN_ERR_ARG, "ttn_eigsolve_history_len: bad mode / d / len");
    std::vector<int64_t> plan;
    const int rc = sweep_plan("ttn_eigsolve_history_len", TTN_ERR_ARG, n_stages, sweep_schedule, nullptr, plan);
    if (rc) return rc;
    *len = eig_hist_len(mode, d, (int64_t)plan.size());
    return TTN_OK;
}

// The penalty of the _ortho entry points (include/ttn_eig_ortho.h): m trains, their host weights [batch][m] and the overlaps out.
// m == 0 (or a null pointer to this) is the plain solve: k_two_site_eig, launched exactly as before the penalty existed.
struct EigOrthoHost { int64_t m; const ttn_tt_t* phi; const double* weights; double* ovl; };

static int two_site_eigsolve(int mode, ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                             const int64_t* rmax_schedule, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                             int64_t hist_len, double* E_out, int64_t* r_out, const EigOrthoHost* oh = nullptr) {
    const char* who = oh ? (mode == 1 ? "ttn_dmrg_eigsolve_ortho" : "ttn_mals_eigsolve_ortho") : (mode == 1 ? "dmrg_eigsolve" : "mals_eigsolve");
    auto err = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
    NEED_INIT();
    if (oh && (oh->m < 0 || oh->m > TTN_EIG_ORTHO_MAX)) return err(TTN_ERR_ARG, "n_ortho outside 0 .. 8");
    const int m_pen = oh ? (int)oh->m : 0;
    if (m_pen && (!oh->phi || !oh->weights || !oh->ovl)) return err(TTN_ERR_ARG, "null phi / weights / ovl");
    for (int j = 0; j < m_pen; ++j) {
        if (!oh->phi[j]) return err(TTN_ERR_ARG, "null handle among phi");
        if (oh->phi[j]->el == 2) return refuse_c64(who);
    }
    F64_ONLY(oh ? who : "two-site eigensolver", {x0, x}, {A});
    if (!A || !x0 || !x) return err(TTN_ERR_ARG, "null handle");
    if (!rmax_schedule || !E_out || !r_out) return err(TTN_ERR_ARG, "null schedule / history buffer");
    if (!same_dims(A->dims, x0->dims) || !same_dims(x0->dims, x->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != x0->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (int rb = op_batch_fits(A, x->batch)) return rb;
    const int d = x0->d;
    if (d < 2) return err(TTN_ERR_UNSUPPORTED, "needs at least two sites");
    if (!(tol >= 0.0) || maxiter < 1 || !(linsolv_tol >= 0.0) || itslv_thresh < 0) return err(TTN_ERR_ARG, "bad tol / linsolv_maxiter / linsolv_tol / itslv_thresh");
    std::vector<int64_t> plan;
    int rc = sweep_plan(who, TTN_ERR_ARG, n_stages, sweep_schedule, rmax_schedule, plan);
    if (rc) return rc;
    if (hist_len != eig_hist_len(mode, d, (int64_t)plan.size())) return err(TTN_ERR_ARG, "hist_len differs from ttn_eigsolve_history_len");
    const int batch = x->batch;
    for (int j = 0; j < m_pen; ++j) {
        const ttn_tt_s* ph = oh->phi[j];
        if (ph == x || ph == x0) return err(TTN_ERR_ARG, "a phi[j] is x or x0");
        if (!same_dims(ph->dims, x->dims)) return err(TTN_ERR_DIMS, "a phi[j] has other dims than x");
        if (ph->batch != batch && ph->batch != 1) return err(TTN_ERR_ARG, "the batch of a phi[j] is neither that of x nor 1");
    }
    for (int64_t k = 0; k < (int64_t)m_pen * batch; ++k)
        if (!std::isfinite(oh->weights[k]) || !(oh->weights[k] > 0.0)) return err(TTN_ERR_ARG, "a weight is not finite or not > 0");
    // ---- every size check before anything is launched ----
    const std::vector<int64_t>& c = x->cap;
    for (int k = 0; k <= d; ++k) if (c[k] < x0->bound[k]) return fail(TTN_ERR_CAPACITY, "rank capacity of the result handle is below the start ranks");
    TwoSiteLayout L = two_site_slots(x0->dims, c, A->rks, nullptr);
    const long long Nmax = L.Nmax, mmax = L.mmax;
    if (mmax > 256) return err(TTN_ERR_UNSUPPORTED, "n_i * capacity above 256 (ranks above 128 for n = 2) is not supported by the SVD core moves");
    if (Nmax > 65536) return err(TTN_ERR_UNSUPPORTED, "two-site problems above 65 536 unknowns are not supported");
    // branch choice (dmrg.jl:237, mals.jl:181): matrix-free if it_solver or N > threshold.  mals_eigsolve does not forward itslv_thresh
    // to K_eigmin_mals (mals.jl:383-390, :403-410), so its threshold is always the default 256 there — restated.
    const long long thresh = mode == 1 ? (long long)itslv_thresh : 256;
    const long long dense_max = it_solver ? 0 : std::min<long long>(TTN_DENSE_LOCAL_MAX, thresh);
    const bool need_lz = it_solver || Nmax > dense_max;
    const long long Kdim = std::min<long long>(Nmax, dense_max);
    EigArgs Rg;
    memset(&Rg, 0, sizeof(Rg));
    MalsArgs& Q = Rg.M;
    AlsArgs& P = Q.L;
    long long& cur = L.cur;
    P.offK = cur; cur += Kdim * Kdim;
    Rg.offEig = cur; cur += 8 + 8 * Kdim;
    if (need_lz) { Rg.offLz = cur; Rg.lz_nmax = Nmax; cur += (TTN_LZ_M + 1 + TTN_LZ_KEEP + L.Rzmax) * Nmax + 5000; }
    P.offPb = cur; cur += Nmax;
    two_site_core_move_blocks(L, Q);
    long long cmax = 1;
    for (int k = 0; k <= d; ++k) cmax = std::max<long long>(cmax, c[k]);
    P.offTm = cur; cur += mmax * cmax;                      // the QR re-orthonormalisation of every core move
    P.offQb = cur; cur += mmax * cmax;
    P.offRb = cur; cur += cmax * cmax;
    P.offTst = cur; cur += ((cmax + QR_NB - 1) / QR_NB) * QR_NB * QR_NB + 64;
    EigOrthoArgs Og;
    memset(&Og, 0, sizeof(Og));
    if (m_pen) {                                            // the overlap chains, the projected vectors and their intermediates
        Og.m = m_pen;
        Og.nmax = Nmax;
        Og.offChain = cur;
        long long qmax = 1;
        for (int j = 0; j < m_pen; ++j) {
            long long q = 1;
            for (int k = 0; k <= d; ++k) q = std::max<long long>(q, oh->phi[j]->bound[k]);
            qmax = std::max(qmax, q);
            Og.slot[j] = cmax * q;
            Og.chain0[j] = cur - Og.offChain;
            cur += 2 * (d + 1) * Og.slot[j];
        }
        Og.offP = cur; cur += (long long)m_pen * Nmax;
        Og.offU = cur; cur += mmax * qmax;
        Og.offW = cur; cur += mmax * qmax;
        Og.offC = cur; cur += 8;
    }
    {
        const size_t need = two_site_bytes(L, batch);
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        if (need > g_scratch.bytes && need - g_scratch.bytes > free_b)
            return err(TTN_ERR_CAPACITY, "the workspace of this capacity and batch (G / H slots, dense K, Lanczos basis, overlap chains) does not fit in device memory");
    }
    if (m_pen) {                                            // ||phi_j|| once per call (k_dot), the last check; then the device tables
        std::vector<double> tab((size_t)2 * batch * m_pen), nn;
        for (int j = 0; j < m_pen; ++j) {
            const ttn_tt_t ph = oh->phi[j];
            nn.assign((size_t)ph->batch, 0.0);
            if ((rc = ttn_dot(ph, ph, nn.data()))) return rc;
            for (int t = 0; t < ph->batch; ++t)
                if (!std::isfinite(nn[t]) || !(nn[t] > 0.0)) return err(TTN_ERR_ARG, "the norm of a phi[j] is zero or not finite");
            for (int t = 0; t < batch; ++t) tab[(size_t)batch * m_pen + (size_t)t * m_pen + j] = 1.0 / std::sqrt(nn[ph->batch == 1 ? 0 : t]);
        }
        for (size_t k = 0; k < (size_t)batch * m_pen; ++k) tab[k] = oh->weights[k];
        if ((rc = g_eig_ortho.ensure(sizeof(double) * 3 * batch * m_pen))) return rc;
        HIPCHK(hipMemcpyAsync(g_eig_ortho.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));            // tab is local
        Og.weight = g_eig_ortho.as<double>();
        Og.inv_norm = Og.weight + (size_t)batch * m_pen;
        Og.ovl = g_eig_ortho.as<double>() + (size_t)2 * batch * m_pen;
        for (int j = 0; j < m_pen; ++j) Og.phi[j] = oh->phi[j]->dev();
    }
    rc = ttn_orthogonalize(x0, 1, x);                       // dmrg.jl:522, mals.jl:355
    if (rc) return rc;
    const int64_t rmax = rmax_schedule[n_stages - 1];
    rc = two_site_prelude(Q, L, A, x, x, tol, rmax, mode, plan);
    if (rc) return rc;
    // device history and Lanczos statistics
    const size_t hn = (size_t)batch * (size_t)hist_len;
    if ((rc = g_hist_E.ensure(sizeof(double) * hn)) || (rc = g_hist_r.ensure(sizeof(long long) * hn)) ||
        (rc = g_lz_iters.ensure(sizeof(int) * batch)) || (rc = g_lz_res.ensure(sizeof(double) * batch)))
        return rc;
    Rg.hist_E = g_hist_E.as<double>(); Rg.hist_r = g_hist_r.as<long long>(); Rg.hist_len = (int)hist_len;
    Rg.lz_all = it_solver ? 1 : 0;
    Rg.lz_above = (int)std::min<long long>(dense_max, 1LL << 30);
    Rg.lz_maxrestart = (int)std::min<int64_t>(maxiter, 1 << 30);
    Rg.lz_tol = linsolv_tol;
    Rg.lz_iters = g_lz_iters.as<int>(); Rg.lz_res = g_lz_res.as<double>();
    if (m_pen) hipLaunchKernelGGL(k_two_site_eig_ortho, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Rg, Og);
    else hipLaunchKernelGGL(k_two_site_eig, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Rg);
    HIPCHK(hipGetLastError());
    if (m_pen) HIPCHK(hipMemcpyAsync(oh->ovl, Og.ovl, sizeof(double) * batch * m_pen, hipMemcpyDeviceToHost, g_stream));
    g_lz_iters_host.assign(batch, 0);
    g_lz_res_host.assign(batch, 0.0);
    std::vector<long long> hr(hn);
    if (hn) {
        HIPCHK(hipMemcpyAsync(E_out, g_hist_E.p, sizeof(double) * hn, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipMemcpyAsync(hr.data(), g_hist_r.p, sizeof(long long) * hn, hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipMemcpyAsync(g_lz_iters_host.data(), g_lz_iters.p, sizeof(int) * batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(g_lz_res_host.data(), g_lz_res.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g_stream));
    unsigned seen = 0;
    rc = take_status(x, seen);                              // synchronises the copies above too
    if (rc) return rc;
    for (size_t k = 0; k < hn; ++k) r_out[k] = (int64_t)hr[k];
    two_site_epilogue(x, mode, plan, mode == 1 ? rmax : 1);
    return status_error(seen, who);
}

int ttn_dmrg_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                      int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh, int64_t hist_len, double* E, int64_t* r_hist) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return two_site_eigsolve(1, A, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, it_solver, maxiter, linsolv_tol, itslv_thresh, hist_len, E, r_hist);
}

int ttn_mals_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                      int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh, int64_t hist_len, double* E, int64_t* r_hist) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return two_site_eigsolve(0, A, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, it_solver, maxiter, linsolv_tol, itslv_thresh, hist_len, E, r_hist);
}

int ttn_dmrg_eigsolve_ortho(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_ortho, const ttn_tt_t* phi, const double* weights, double tol, int64_t n_stages,
                            const int64_t* sweep_schedule, const int64_t* rmax_schedule, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                            int64_t hist_len, double* E, int64_t* r_hist, double* ovl) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_dmrg_eigsolve_ortho")) return rb;
    const EigOrthoHost oh{n_ortho, phi, weights, ovl};
    return two_site_eigsolve(1, A, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, it_solver, maxiter, linsolv_tol, itslv_thresh, hist_len, E, r_hist, &oh);
}

int ttn_mals_eigsolve_ortho(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_ortho, const ttn_tt_t* phi, const double* weights, double tol, int64_t n_stages,
                            const int64_t* sweep_schedule, const int64_t* rmax_schedule, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                            int64_t hist_len, double* E, int64_t* r_hist, double* ovl) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_mals_eigsolve_ortho")) return rb;
    const EigOrthoHost oh{n_ortho, phi, weights, ovl};
    return two_site_eigsolve(0, A, x0, x, tol, n_stages, sweep_schedule, rmax_schedule, it_solver, maxiter, linsolv_tol, itslv_thresh, hist_len, E, r_hist, &oh);
}

int ttn_eigsolve_stats(int64_t batch, int64_t* lanczos_applies, double* lanczos_residual) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!lanczos_applies || !lanczos_residual || batch < 0 || (size_t)batch > g_lz_iters_host.size())
        return fail(TTN_ERR_ARG, "ttn_eigsolve_stats: no eigensolve of that batch size has run");
    for (int64_t t = 0; t < batch; ++t) { lanczos_applies[t] = g_lz_iters_host[(size_t)t]; lanczos_residual[t] = g_lz_res_host[(size_t)t]; }
    return TTN_OK;
}

// ---- core gradients (csrc/ttn_grad_kernels.h) ------------------------------------------------------------------------------------
// What the four calls check alike before anything is launched: Float64 handles of equal dims and batch, trains below 2^31 doubles.
static int grad_common(const char* who, std::initializer_list<const ttn_tt_s*> tts) {
    const ttn_tt_s* first = nullptr;
    for (const ttn_tt_s* h : tts) {
        if (!h) continue;
        if (!first) first = h;
        if (!same_dims(first->dims, h->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
        if (first->batch != h->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    }
    if (any_c64(tts)) return refuse_c64(who);
    for (const ttn_tt_s* h : tts)
        if (h && h->stride >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, (std::string(who) + ": a train of 2^31 doubles or more").c_str());
    return TTN_OK;
}
// dst becomes a tangent of src: src's ranks (copied on the device), its host-side bounds, gauge flags 0
static void grad_tangent_of(ttn_tt_t dst, ttn_tt_t src) {
    hipLaunchKernelGGL(k_ranks_copy, dim3(src->batch), dim3(64), 0, g_stream, dst->dev(), src->dev());
    dst->bound = src->bound;
    std::fill(dst->ot.begin(), dst->ot.end(), 0);
}
// `batch` host doubles into half `slot` of g_grad_coef (null: no copy, the kernel takes 1).  Synchronises: `v` is caller memory.
static int grad_coef(const double* v, int batch, int slot, const double*& dev) {
    dev = nullptr;
    if (!v) return TTN_OK;
    const int rc = g_grad_coef.ensure(sizeof(double) * 2 * (size_t)batch);
    if (rc) return rc;
    double* p = g_grad_coef.as<double>() + (size_t)slot * batch;
    HIPCHK(hipMemcpyAsync(p, v, sizeof(double) * batch, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    dev = p;
    return TTN_OK;
}

int ttn_dot_pullback(ttn_tt_t a, ttn_tt_t b, const double* delta, ttn_tt_t abar, ttn_tt_t bbar, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!a || !b) return fail(TTN_ERR_ARG, "ttn_dot_pullback: null handle");
    if (!abar && !bbar) return fail(TTN_ERR_ARG, "ttn_dot_pullback: neither abar nor bbar is given");
    if ((abar && (abar == a || abar == b || abar == bbar)) || (bbar && (bbar == a || bbar == b)))
        return fail(TTN_ERR_ARG, "ttn_dot_pullback: an output must not alias an operand or the other output");
    int rc = grad_common("ttn_dot_pullback", {a, b, abar, bbar});
    if (rc) return rc;
    const int d = a->d, batch = a->batch;
    if (d > DOT_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_dot_pullback: chains longer than 480 sites are not supported");
    for (int m = 0; m <= d; ++m)
        if ((abar && abar->cap[m] < a->bound[m]) || (bbar && bbar->cap[m] < b->bound[m]))
            return fail(TTN_ERR_CAPACITY, "ttn_dot_pullback: destination capacity too small");
    // workspace per train: both chains with every state, 2 (d + 1) W doubles, W = max_m r^A_m r^B_m, and one GEMM intermediate per chain
    long long W = 1, ramax = 1, rbmax = 1, nmax = 1, tiles = 1;
    for (int m = 0; m <= d; ++m) {
        W = std::max<long long>(W, a->bound[m] * b->bound[m]);
        ramax = std::max<long long>(ramax, a->bound[m]); rbmax = std::max<long long>(rbmax, b->bound[m]);
    }
    for (int k = 0; k < d; ++k) nmax = std::max<long long>(nmax, a->dims[k]);
    W = (W + 1) & ~1LL;
    const long long tsz = (nmax * ramax * rbmax + 1) & ~1LL;
    for (int k = 0; k < d; ++k) {
        if (abar) tiles = std::max<long long>(tiles, ((a->bound[k] + 15) / 16) * ((a->bound[k + 1] + 63) / 64));
        if (bbar) tiles = std::max<long long>(tiles, ((b->bound[k] + 15) / 16) * ((b->bound[k + 1] + 63) / 64));
    }
    if (tiles >= (1LL << 31) || batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_dot_pullback: more than 2^31 output tiles in one core, or more than 65535 trains");
    const size_t per_train = (size_t)(2 * (d + 1) * W + 2 * tsz);
    if ((rc = scratch_take(sizeof(double) * per_train * batch))) return rc;
    if ((rc = g_dout.ensure(sizeof(double) * batch))) return rc;
    const double* d_delta = nullptr;
    if ((rc = grad_coef(delta, batch, 0, d_delta))) return rc;
    if (abar) grad_tangent_of(abar, a);
    if (bbar) grad_tangent_of(bbar, b);
    GradChainArgs C_;
    C_.a = a->dev(); C_.b = b->dev();
    C_.env = g_scratch.as<double>();
    C_.tbuf = C_.env + (size_t)2 * (d + 1) * W * batch;
    C_.W = W; C_.tsz = tsz;
    C_.out = out ? g_dout.as<double>() : nullptr;
    hipLaunchKernelGGL(k_grad_chain, dim3(batch, 2), dim3(TTN_WG), DOT_LDS_BYTES(d), g_stream, C_);
    HIPCHK(hipGetLastError());
    GradSandArgs S_;
    S_.a = a->dev(); S_.b = b->dev();
    S_.abar = abar ? abar->dev() : TTDev{}; S_.bbar = bbar ? bbar->dev() : TTDev{};
    S_.env = C_.env; S_.W = W; S_.delta = d_delta;
    hipLaunchKernelGGL(k_grad_sandwich, dim3((unsigned)tiles, 2 * d, batch), dim3(GRAD_SW_TB), 0, g_stream, S_);
    HIPCHK(hipGetLastError());
    if (out) {
        HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return TTN_OK;
}

// The pullback of <x, A y> on the three-layer environments (include/ttn_expect_grad.h, csrc/ttn_expect_grad_kernels.h): A y is never formed.
int ttn_sandwich_pullback(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, const double* delta, ttn_tt_t xbar, ttn_tt_t ybar, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !A || !y) return fail(TTN_ERR_ARG, "ttn_sandwich_pullback: null handle");
    if (!xbar && !ybar) return fail(TTN_ERR_ARG, "ttn_sandwich_pullback: neither xbar nor ybar is given");
    if ((xbar && (xbar == x || xbar == y || xbar == ybar)) || (ybar && (ybar == x || ybar == y)))
        return fail(TTN_ERR_ARG, "ttn_sandwich_pullback: an output must not alias an operand or the other output");
    if (!same_dims(A->dims, x->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    int rc = grad_common("ttn_sandwich_pullback", {x, y, xbar, ybar});
    if (rc) return rc;
    if (A->el == 2) return refuse_c64("ttn_sandwich_pullback");
    const int d = x->d, batch = x->batch;
    if (int rb = op_batch_fits(A, batch)) return rb;
    if (d > EXPECT_MAX_D) return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich_pullback: chains longer than 480 sites are not supported");
    if (A->off.back() >= (1LL << 31)) return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich_pullback: an operator of 2^31 doubles or more");
    if (batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich_pullback: more than 65535 trains");
    for (int m = 0; m <= d; ++m)
        if ((xbar && xbar->cap[m] < x->bound[m]) || (ybar && ybar->cap[m] < y->bound[m]))
            return fail(TTN_ERR_CAPACITY, "ttn_sandwich_pullback: destination capacity too small");
    long long rxmax = 1, rymax = 1, Rmax = 1, nmax = 1, W = 1;
    bool wbig = false;
    for (int m = 0; m <= d; ++m) {
        rxmax = std::max<long long>(rxmax, x->bound[m]); rymax = std::max<long long>(rymax, y->bound[m]); Rmax = std::max<long long>(Rmax, A->rks[m]);
        if (x->bound[m] >= (1LL << 31) || y->bound[m] >= (1LL << 31) || A->rks[m] >= (1LL << 31) || x->bound[m] * y->bound[m] >= (1LL << 31)) wbig = true;
        else W = std::max<long long>(W, x->bound[m] * y->bound[m] * A->rks[m]);
    }
    bool qtt = Rmax <= EXPECT_QTT_OPR_MAX;
    for (int k = 0; k < d; ++k) { nmax = std::max<long long>(nmax, x->dims[k]); qtt = qtt && x->dims[k] == 2; }
    // 32-bit element offsets in the workgroup GEMM, as in ttn_sandwich
    if (wbig || rxmax * rymax >= (1LL << 31) || rxmax * rymax * Rmax >= (1LL << 31) || (2 + 2 * nmax) * rxmax * rymax * Rmax >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_sandwich_pullback: ranks too large (the three-layer state of one train reaches 2^31 doubles)");
    // workspace per train (doubles): 2 (d + 1) W  both chains with every state, W = max_m rx_m R_m ry_m (even)
    //                              + 2 wsz        per chain: U and V of a GEMM site, 2 nmax S with S = rxmax Rmax rymax, or the Rmax 64 x 64
    //                                             images of the on-chip G chain
    //                              + 4 d nmax S   T1 and T2 of the 2 d outputs of the general gradient route — absent when every train is
    //                                             known on the host to be of the on-chip class
    W = (W + 1) & ~1LL;
    const long long S = rxmax * Rmax * rymax;
    const long long wsz = (std::max<long long>(2 * nmax * S, qtt ? Rmax * EXPECT_IMG_STATE : 0) + 1) & ~1LL;
    const bool all_chip = qtt && rxmax <= EXPECT_QTT_RMAX && rymax <= EXPECT_QTT_RMAX;
    const long long gw = all_chip ? 0 : 4LL * d * nmax * S;
    // and, behind it all, one 32-bit route word per train.
    const size_t per_train = (size_t)(2LL * (d + 1) * W + 2 * wsz + gw);
    if ((rc = scratch_take(sizeof(double) * per_train * batch + sizeof(int) * batch))) return rc;
    if ((rc = g_dout.ensure(sizeof(double) * batch))) return rc;
    const double* d_delta = nullptr;
    if ((rc = grad_coef(delta, batch, 0, d_delta))) return rc;
    if (xbar) grad_tangent_of(xbar, x);
    if (ybar) grad_tangent_of(ybar, y);
    ExpGradArgs P;
    P.x = x->dev(); P.y = y->dev(); P.A = A->dev();
    P.xbar = xbar ? xbar->dev() : TTDev{}; P.ybar = ybar ? ybar->dev() : TTDev{};
    P.env = g_scratch.as<double>();
    P.work = P.env + (size_t)2 * (d + 1) * W * batch;
    P.gwork = all_chip ? nullptr : P.work + (size_t)2 * wsz * batch;
    P.route = (int*)(P.env + per_train * batch);
    P.W = W; P.wsz = wsz; P.S = S; P.nmax = (int)nmax;
    P.delta = d_delta;
    P.out = out ? g_dout.as<double>() : nullptr;
    const int rm = qtt ? (int)Rmax : 0;
    const dim3 cgrid(batch, 2), cblock(TTN_WG);
    const size_t clds = EXPECT_LDS_BYTES(d);
    const dim3 qgrid(EXPECT_QTT_RMAX / 16, 2 * d, batch), qblock(EXPGRAD_TB);
    switch (rm) {
        case 1: hipLaunchKernelGGL(k_expgrad_chain<1>, cgrid, cblock, clds, g_stream, P); hipLaunchKernelGGL(k_expgrad_core<1>, qgrid, qblock, 0, g_stream, P); break;
        case 2: hipLaunchKernelGGL(k_expgrad_chain<2>, cgrid, cblock, clds, g_stream, P); hipLaunchKernelGGL(k_expgrad_core<2>, qgrid, qblock, 0, g_stream, P); break;
        case 3: hipLaunchKernelGGL(k_expgrad_chain<3>, cgrid, cblock, clds, g_stream, P); hipLaunchKernelGGL(k_expgrad_core<3>, qgrid, qblock, 0, g_stream, P); break;
        case 4: hipLaunchKernelGGL(k_expgrad_chain<4>, cgrid, cblock, clds, g_stream, P); hipLaunchKernelGGL(k_expgrad_core<4>, qgrid, qblock, 0, g_stream, P); break;
        case 5: hipLaunchKernelGGL(k_expgrad_chain<5>, cgrid, cblock, clds, g_stream, P); hipLaunchKernelGGL(k_expgrad_core<5>, qgrid, qblock, 0, g_stream, P); break;
        default: hipLaunchKernelGGL(k_expgrad_chain<0>, cgrid, cblock, clds, g_stream, P); break;
    }
    HIPCHK(hipGetLastError());
    if (!all_chip) {
        const dim3 ggrid(2 * d, batch);
        const size_t glds = sizeof(double) * GEMM_LDS_TOTAL;
        if (qtt) hipLaunchKernelGGL(k_expgrad_core_gen<true>, ggrid, cblock, glds, g_stream, P);
        else hipLaunchKernelGGL(k_expgrad_core_gen<false>, ggrid, cblock, glds, g_stream, P);
        HIPCHK(hipGetLastError());
    }
    if (out) {
        HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return TTN_OK;
}

int ttn_apply_pullback(ttn_tto_t A, ttn_tt_t x, ttn_tt_t ybar, ttn_tt_t xbar) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !x || !ybar || !xbar) return fail(TTN_ERR_ARG, "ttn_apply_pullback: null handle");
    if (int rb = single_op(A, "ttn_apply_pullback")) return rb;
    if (xbar == x || xbar == ybar) return fail(TTN_ERR_ARG, "ttn_apply_pullback: the output must not alias an operand");
    if (!same_dims(A->dims, x->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    int rc = grad_common("ttn_apply_pullback", {x, ybar, xbar});
    if (rc) return rc;
    if (A->el == 2) return refuse_c64("ttn_apply_pullback");
    const int d = x->d, batch = x->batch;
    for (int m = 0; m <= d; ++m) if (xbar->cap[m] < x->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_apply_pullback: destination capacity too small");
    for (int m = 0; m <= d; ++m) if (ybar->cap[m] < A->rks[m]) return fail(TTN_ERR_CAPACITY, "ttn_apply_pullback: ybar cannot hold the ranks R .* x");
    long long items = 1, amax_ = 0;
    for (int k = 0; k < d; ++k) {
        if (stream_fibres_too_many((long long)x->dims[k] * x->bound[k] * x->bound[k + 1]) || stream_fibres_too_many((long long)ybar->cap[k] * ybar->cap[k + 1]))
            return fail(TTN_ERR_UNSUPPORTED, "ttn_apply_pullback: 2^31 or more fibres in one core (32-bit element indices)");
        items = std::max<long long>(items, x->dims[k] == 2 ? x->bound[k] * ((x->bound[k + 1] + TTN_APB_K - 1) / TTN_APB_K) : x->dims[k] * x->bound[k] * x->bound[k + 1]);
        amax_ = std::max<long long>(amax_, (long long)A->dims[k] * A->dims[k] * A->rks[k] * A->rks[k + 1]);
    }
    if (batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_apply_pullback: more than 65535 trains");
    const int lds_a = amax_ <= TTN_APPLY_LDS_DOUBLES ? (int)amax_ : 0;
    grad_tangent_of(xbar, x);
    hipLaunchKernelGGL(k_apply_pullback, stream_grid(items, d, batch), dim3(TTN_STREAM_TB), sizeof(double) * (size_t)lds_a, g_stream, A->dev(), x->dev(),
                       ybar->dev(), xbar->dev(), lds_a, xbar->d_status);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_tt_cores_axpby(const double* alpha, ttn_tt_t x, const double* beta, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y) return fail(TTN_ERR_ARG, "ttn_tt_cores_axpby: null handle");
    int rc = grad_common("ttn_tt_cores_axpby", {x, y});
    if (rc) return rc;
    const int d = x->d, batch = x->batch;
    for (int m = 0; m <= d; ++m) if (y->cap[m] < x->bound[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_cores_axpby: destination capacity too small");
    if (batch > 65535) return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_cores_axpby: more than 65535 trains");
    const double* d_alpha = nullptr; const double* d_beta = nullptr;
    if ((rc = grad_coef(alpha, batch, 0, d_alpha))) return rc;
    if ((rc = grad_coef(beta, batch, 1, d_beta))) return rc;
    long long maxsz = 1;
    for (int k = 0; k < d; ++k) maxsz = std::max<long long>(maxsz, (long long)x->dims[k] * x->bound[k] * x->bound[k + 1]);
    hipLaunchKernelGGL(k_cores_axpby, stream_grid((maxsz + 3) / 4, d, batch), dim3(TTN_STREAM_TB), 0, g_stream, x->dev(), y->dev(), d_alpha, d_beta, y->d_status);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_tt_cores_dot(ttn_tt_t x, ttn_tt_t y, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y || !out) return fail(TTN_ERR_ARG, "ttn_tt_cores_dot: null pointer");
    int rc = grad_common("ttn_tt_cores_dot", {x, y});
    if (rc) return rc;
    if ((rc = g_dout.ensure(sizeof(double) * x->batch))) return rc;
    hipLaunchKernelGGL(k_cores_dot, dim3(x->batch), dim3(TTN_WG), 0, g_stream, x->dev(), y->dev(), g_dout.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * x->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// kernel unit-test hook: C (m x n, row-major, host) = alpha * op(A) * op(B) + beta * C through wg_gemm on the device
int ttn_selftest_gemm(int64_t m, int64_t n, int64_t k, const double* A, const double* B, double* C, double alpha, double beta,
                      int ta, int tb) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !B || !C || m < 1 || n < 1 || k < 1) return fail(TTN_ERR_ARG, "bad argument");
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    HIPCHK(hipMalloc((void**)&dA, sizeof(double) * m * k));
    HIPCHK(hipMalloc((void**)&dB, sizeof(double) * k * n));
    HIPCHK(hipMalloc((void**)&dC, sizeof(double) * m * n));
    HIPCHK(hipMemcpyAsync(dA, A, sizeof(double) * m * k, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dB, B, sizeof(double) * k * n, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dC, C, sizeof(double) * m * n, hipMemcpyHostToDevice, g_stream));   // C is an accumulator (beta * C): uploaded whole; no
                                                                                              // allocation of this hook is left for poison mode to fill
    if (getenv("TTN_WG512_SELFTEST") && atoi(getenv("TTN_WG512_SELFTEST"))) {       // the same test against the 512-thread build
        const int rc512 = ttn_wg512_selftest_gemm((int)m, (int)n, (int)k, dA, dB, dC, alpha, beta, ta, tb, g_stream);
        if (rc512) return hipfail((hipError_t)rc512, "k_selftest_gemm (512-thread build)");
    } else {
    hipLaunchKernelGGL(k_selftest_gemm, dim3(1), dim3(TTN_WG), sizeof(double) * GEMM_LDS_TOTAL, g_stream, (int)m, (int)n, (int)k,
                       dA, dB, dC, alpha, beta, ta, tb);
    HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(C, dC, sizeof(double) * m * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    hipFree(dA); hipFree(dB); hipFree(dC);
    return TTN_OK;
}

// kernel unit-test hook of wg_syrk2: G_i (p_i x p_i, row-major, host, in/out) = alpha_i A_i A_i^T, both products in ONE single-workgroup
// launch; pair = 0 computes them by two wg_syrk calls instead (the unpaired reference)
int ttn_selftest_syrk2(int64_t p1, int64_t q1, const double* A1, double* G1, double alpha1, int ta1,
                       int64_t p2, int64_t q2, const double* A2, double* G2, double alpha2, int ta2, int pair) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A1 || !G1 || !A2 || !G2 || p1 < 1 || q1 < 1 || p2 < 1 || q2 < 1 || p1 > 4096 || p2 > 4096 || q1 > 16384 || q2 > 16384)
        return fail(TTN_ERR_ARG, "bad argument");
    double *dA1 = nullptr, *dA2 = nullptr, *dG1 = nullptr, *dG2 = nullptr;
    HIPCHK(hipMalloc((void**)&dA1, sizeof(double) * p1 * q1));
    HIPCHK(hipMalloc((void**)&dA2, sizeof(double) * p2 * q2));
    HIPCHK(hipMalloc((void**)&dG1, sizeof(double) * p1 * p1));
    HIPCHK(hipMalloc((void**)&dG2, sizeof(double) * p2 * p2));
    HIPCHK(hipMemcpyAsync(dA1, A1, sizeof(double) * p1 * q1, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dA2, A2, sizeof(double) * p2 * q2, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dG1, G1, sizeof(double) * p1 * p1, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dG2, G2, sizeof(double) * p2 * p2, hipMemcpyHostToDevice, g_stream));   // G_i are in/out by contract and uploaded whole (poison mode: nothing to fill)
    if (getenv("TTN_WG512_SELFTEST") && atoi(getenv("TTN_WG512_SELFTEST"))) {       // the same test against the 512-thread build
        const int rc512 = ttn_wg512_selftest_syrk2((int)p1, (int)q1, dA1, dG1, alpha1, ta1, (int)p2, (int)q2, dA2, dG2, alpha2, ta2, pair, g_stream);
        if (rc512) return hipfail((hipError_t)rc512, "k_selftest_syrk2 (512-thread build)");
    } else {
        hipLaunchKernelGGL(k_selftest_syrk2, dim3(1), dim3(TTN_WG), sizeof(double) * GEMM_LDS_TOTAL, g_stream, (int)p1, (int)q1, dA1, dG1, alpha1, ta1,
                           (int)p2, (int)q2, dA2, dG2, alpha2, ta2, pair);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(G1, dG1, sizeof(double) * p1 * p1, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(G2, dG2, sizeof(double) * p2 * p2, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    hipFree(dA1); hipFree(dA2); hipFree(dG1); hipFree(dG2);
    return TTN_OK;
}

// kernel unit-test hook of wg_gemm_ra2: C_i (m_i x n_i, host, in/out) = alpha_i A_i B_i, both products in ONE single-workgroup launch; f_i & 1 / 2 / 4:
// A_i / B_i / C_i stored transposed; pair = 0 computes them by two wg_gemm_ra calls instead (the unpaired reference)
int ttn_selftest_gemm_ra2(int64_t m1, int64_t n1, int64_t k1, const double* A1, const double* B1, double* C1, double alpha1, int f1,
                          int64_t m2, int64_t n2, int64_t k2, const double* A2, const double* B2, double* C2, double alpha2, int f2, int pair) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    const int64_t dm[2] = {m1, m2}, dn[2] = {n1, n2}, dk[2] = {k1, k2};
    const double* hA[2] = {A1, A2};
    const double* hB[2] = {B1, B2};
    double* hC[2] = {C1, C2};
    for (int i = 0; i < 2; ++i)
        if (!hA[i] || !hB[i] || !hC[i] || dm[i] < 1 || dn[i] < 1 || dk[i] < 1 || dm[i] > 4096 || dn[i] > 4096 || dk[i] > 4096) return fail(TTN_ERR_ARG, "bad argument");
    double *dA[2] = {nullptr, nullptr}, *dB[2] = {nullptr, nullptr}, *dC[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipMalloc((void**)&dA[i], sizeof(double) * dm[i] * dk[i]));
        HIPCHK(hipMalloc((void**)&dB[i], sizeof(double) * dk[i] * dn[i]));
        HIPCHK(hipMalloc((void**)&dC[i], sizeof(double) * dm[i] * dn[i]));
        HIPCHK(hipMemcpyAsync(dA[i], hA[i], sizeof(double) * dm[i] * dk[i], hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipMemcpyAsync(dB[i], hB[i], sizeof(double) * dk[i] * dn[i], hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipMemcpyAsync(dC[i], hC[i], sizeof(double) * dm[i] * dn[i], hipMemcpyHostToDevice, g_stream));   // in/out by contract, uploaded whole (poison mode: nothing to fill)
    }
    if (getenv("TTN_WG512_SELFTEST") && atoi(getenv("TTN_WG512_SELFTEST"))) {       // the same test against the 512-thread build
        const int rc512 = ttn_wg512_selftest_gemm_ra2((int)m1, (int)n1, (int)k1, dA[0], dB[0], dC[0], alpha1, f1, (int)m2, (int)n2, (int)k2, dA[1], dB[1], dC[1],
                                                      alpha2, f2, pair, g_stream);
        if (rc512) return hipfail((hipError_t)rc512, "k_selftest_gemm_ra2 (512-thread build)");
    } else {
        hipLaunchKernelGGL(k_selftest_gemm_ra2, dim3(1), dim3(TTN_WG), sizeof(double) * GEMM_LDS_TOTAL, g_stream, (int)m1, (int)n1, (int)k1, dA[0], dB[0], dC[0],
                           alpha1, f1, (int)m2, (int)n2, (int)k2, dA[1], dB[1], dC[1], alpha2, f2, pair);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < 2; ++i) HIPCHK(hipMemcpyAsync(hC[i], dC[i], sizeof(double) * dm[i] * dn[i], hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int i = 0; i < 2; ++i) { hipFree(dA[i]); hipFree(dB[i]); hipFree(dC[i]); }
    return TTN_OK;
}

// kernel unit-test hook of the dense local solve: K x = rhs by the blocked LU with partial pivoting.  form 0: wg_lu_solve in one
// workgroup (what k_als_linsolve / k_mals_linsolve run); form 1: the stages of csrc/ttn_als_grid.h through lu_grid_solve (what
// als_grid_path runs).  Returns 0, 1 for an exactly zero pivot column, or a TTN_ERR_* code.
int ttn_selftest_lu_solve(int64_t N, const double* K, const double* rhs, double* x_out, int64_t* piv_out, int form) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!K || !rhs || !x_out || !piv_out || N < 1 || (form != 0 && form != 1) || N > (form == 0 ? TTN_DENSE_LOCAL_MAX_ALS : 8192))
        return fail(TTN_ERR_ARG, "ttn_selftest_lu_solve: need 1 <= N <= 2048 (form 0) / 8192 (form 1) and form 0 or 1");
    NEED_INIT();
    { const int rc = g_lu_flag.ensure(sizeof(int)); if (rc) return rc; }
    int* d_flag = g_lu_flag.as<int>();
    double *dK = nullptr, *dR = nullptr;
    int* dP = nullptr;
    HIPCHK(hipMalloc((void**)&dK, sizeof(double) * N * N));
    HIPCHK(hipMalloc((void**)&dR, sizeof(double) * N));
    HIPCHK(hipMalloc((void**)&dP, sizeof(int) * N));
    HIPCHK(hipMemcpyAsync(dK, K, sizeof(double) * N * N, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dR, rhs, sizeof(double) * N, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemsetAsync(dP, 0xff, sizeof(int) * N, g_stream));                     // -1: a column the elimination never reached — a sentinel the
                                                                                     // caller reads by contract, so it stays in poison mode; K and rhs are uploaded whole
    HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), g_stream));
    if (form == 0) hipLaunchKernelGGL(k_selftest_lu, dim3(1), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, (int)N, dK, dR, dP, d_flag);
    else lu_grid_solve(dK, dR, (int)N, dP, d_flag);
    HIPCHK(hipGetLastError());
    std::vector<int> h_piv(N);
    int h_flag = 0;
    HIPCHK(hipMemcpyAsync(x_out, dR, sizeof(double) * N, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(h_piv.data(), dP, sizeof(int) * N, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    hipFree(dK); hipFree(dR); hipFree(dP);
    for (int64_t j = 0; j < N; ++j) piv_out[j] = h_piv[j];
    return h_flag ? 1 : 0;
}

// kernel unit-test hook of the matrix-free two-site operator: out = 1/2 (K + K^T) v through wg_two_site_apply, K[(ab,cd),(ef,gh)] =
// sum_z G[ab,ef,z] H[z,cd,gh].  G (na, na, Rz) column-major, H (Rz, nb, nb) with z fastest, v and out na x nb column-major; all host.
int ttn_selftest_two_site_apply(int64_t na, int64_t nb, int64_t Rz, const double* G, const double* H, const double* v, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!G || !H || !v || !out || na < 1 || nb < 1 || Rz < 1 || na > 256 || nb > 256 || Rz > 64)
        return fail(TTN_ERR_ARG, "ttn_selftest_two_site_apply: need 1 <= na, nb <= 256 and 1 <= Rz <= 64");
    NEED_INIT();
    const size_t N = (size_t)na * nb;
    double *dG = nullptr, *dH = nullptr, *dv = nullptr, *dout = nullptr, *dW = nullptr;
    HIPCHK(hipMalloc((void**)&dG, sizeof(double) * na * na * Rz));
    HIPCHK(hipMalloc((void**)&dH, sizeof(double) * nb * nb * Rz));
    HIPCHK(hipMalloc((void**)&dv, sizeof(double) * N));
    HIPCHK(hipMalloc((void**)&dout, sizeof(double) * N));
    HIPCHK(hipMalloc((void**)&dW, sizeof(double) * N * Rz));
    HIPCHK(hipMemcpyAsync(dG, G, sizeof(double) * na * na * Rz, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dH, H, sizeof(double) * nb * nb * Rz, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dv, v, sizeof(double) * N, hipMemcpyHostToDevice, g_stream));
    // out is written whole, W is workspace: zeros / raw by default, the pattern in poison mode
    { int rc; if ((rc = fresh_fill(dout, sizeof(double) * N, true)) || (rc = fresh_fill(dW, sizeof(double) * N * Rz, false))) return rc; }
    hipLaunchKernelGGL(k_selftest_two_site_apply, dim3(1), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, (int)na, (int)nb, (int)Rz, dG, dH, dv, dout, dW);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * N, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    hipFree(dG); hipFree(dH); hipFree(dv); hipFree(dout); hipFree(dW);
    return TTN_OK;
}

// self-test of the 128 x 128 symmetric eigensolver of the Gram route: G (host, column-major) -> sig[nev] = sqrt(eigenvalues)
// descending, X[128 * r] = sqrt(lam_j) u_j, device clock ticks of the whole routine and its return code
int ttn_selftest_eig128(const double* G, int64_t n, int64_t r, int64_t nev, double* sig, double* X, int64_t* ticks_rc) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!G || !sig || !X || (n != 64 && n != 128) || r < 1 || r > 64 || nev < r || nev > n) return fail(TTN_ERR_ARG, "bad argument");
    double *dG = nullptr, *dV = nullptr, *dS = nullptr, *dX = nullptr;
    long long* dC = nullptr;
    HIPCHK(hipMalloc((void**)&dG, sizeof(double) * 128 * 128));
    HIPCHK(hipMalloc((void**)&dV, sizeof(double) * 128 * 128));
    HIPCHK(hipMalloc((void**)&dS, sizeof(double) * 128));
    HIPCHK(hipMalloc((void**)&dX, sizeof(double) * 128 * 64));
    HIPCHK(hipMalloc((void**)&dC, sizeof(long long) * 2));
    // X, sig and the counters are outputs, V is workspace; none is an accumulator.  G is 128 x 128 however small n is: the routine is handed
    // the n x n block only, so the rest is slack
    if (g_poison) { const int rc = poison_fill(dG, sizeof(double) * 128 * 128); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(dG, G, sizeof(double) * n * n, hipMemcpyHostToDevice, g_stream));
    { int rc; if ((rc = fresh_fill(dX, sizeof(double) * 128 * 64, true)) || (rc = fresh_fill(dV, sizeof(double) * 128 * 128, false)) ||
                  (rc = fresh_fill(dS, sizeof(double) * 128, false)) || (rc = fresh_fill(dC, sizeof(long long) * 2, false))) return rc; }
    if (getenv("TTN_WG512_SELFTEST") && atoi(getenv("TTN_WG512_SELFTEST"))) {
        const int rc512 = ttn_wg512_selftest_eig(dG, dV, (int)n, (int)r, (int)nev, dS, dX, dC, g_stream);
        if (rc512) return hipfail((hipError_t)rc512, "k_selftest_eig128 (512-thread build)");
    } else {
    hipLaunchKernelGGL(k_selftest_eig128, dim3(1), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, dG, dV, (int)n, (int)r, (int)nev, dS, dX, dC);
    HIPCHK(hipGetLastError());
    }
    long long hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(sig, dS, sizeof(double) * nev, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(X, dX, sizeof(double) * 128 * r, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(hc, dC, sizeof(hc), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (ticks_rc) { ticks_rc[0] = hc[0]; ticks_rc[1] = hc[1]; }
    hipFree(dG); hipFree(dV); hipFree(dS); hipFree(dX); hipFree(dC);
    return TTN_OK;
}

// self-test of the dense eigen routine of the two-site eigensolvers: A (host, N x N column-major, symmetric) -> lam[k] ascending, Y[N * k]
// the orthonormal eigenvectors, computed by one workgroup calling wg_sym_eig_smallest as k_two_site_eig does (ld = N, 3N + 5N k scratch)
int ttn_selftest_sym_eig(int64_t N, int64_t k, const double* A, double* lam, double* Y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!A || !lam || !Y || N < 1 || N > TTN_DENSE_LOCAL_MAX || k < 1 || k > std::min<int64_t>(N, TTN_NWAVES))
        return fail(TTN_ERR_ARG, "ttn_selftest_sym_eig: need 1 <= N <= 2048 and 1 <= k <= min(N, 16)");
    NEED_INIT();
    double *dA = nullptr, *dL = nullptr, *dY = nullptr, *dW = nullptr;
    HIPCHK(hipMalloc((void**)&dA, sizeof(double) * N * N));
    HIPCHK(hipMalloc((void**)&dL, sizeof(double) * k));
    HIPCHK(hipMalloc((void**)&dY, sizeof(double) * N * k));
    HIPCHK(hipMalloc((void**)&dW, sizeof(double) * (3 * N + 5 * N * k)));
    HIPCHK(hipMemcpyAsync(dA, A, sizeof(double) * N * N, hipMemcpyHostToDevice, g_stream));
    // lam and Y are written whole, W is the routine's workspace (a slice of the per-call workspace in production)
    { int rc; if ((rc = fresh_fill(dY, sizeof(double) * N * k, true)) || (rc = fresh_fill(dL, sizeof(double) * k, false)) ||
                  (rc = fresh_fill(dW, sizeof(double) * (3 * N + 5 * N * k), false))) return rc; }
    hipLaunchKernelGGL(k_selftest_sym_eig, dim3(1), dim3(TTN_WG), 0, g_stream, (int)N, (int)k, dA, dL, dY, dW);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(lam, dL, sizeof(double) * k, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(Y, dY, sizeof(double) * N * k, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    hipFree(dA); hipFree(dL); hipFree(dY); hipFree(dW);
    return TTN_OK;
}

// Poison mode (ttn_host_core.h) and the two probes that let a test prove the fills happen.  Host side only.
int ttn_selftest_poison(int on, uint64_t pattern) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    g_poison = on != 0;
    g_poison_pat = g_poison ? (unsigned long long)pattern : 0ULL;
    return TTN_OK;
}
// Takes `nbytes` of the per-call workspace as an entry point does; the first 8 bytes and the last whole 8-byte word of the WHOLE buffer.
int ttn_selftest_workspace_peek(int64_t nbytes, uint64_t* out_first8, uint64_t* out_last8) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (nbytes < 8 || !out_first8 || !out_last8) return fail(TTN_ERR_ARG, "ttn_selftest_workspace_peek: need nbytes >= 8 and two outputs");
    const int rc = scratch_take((size_t)nbytes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out_first8, g_scratch.p, 8, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(out_last8, g_scratch.as<char>() + (g_scratch.bytes / 8 - 1) * 8, 8, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}
// Raw read of n doubles of train b's arena from `offset` on (slot offsets: the handle's layout, include/ttn.h), live or slack alike.
int ttn_selftest_tt_peek(ttn_tt_t h, int64_t b, int64_t offset, int64_t n, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!h || !out || b < 0 || b >= h->batch || offset < 0 || n < 0 || offset > h->stride || n > h->stride - offset) return fail(TTN_ERR_ARG, "ttn_selftest_tt_peek: bad argument");
    if (n) HIPCHK(hipMemcpyAsync(out, h->d_data + (size_t)b * h->stride + offset, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// ---- TDVP local contractions (src/solvers/tdvp.jl:29-43, :205-208), batched, real or complex -------------------------------------
// Device-pointer forms: every tensor is an array of `batch` column-major tensors laid out back to back (stride = its size; M may be
// shared by the batch: m_shared != 0).  The host forms (…_f64) stage host arrays of the same layout through the device.
static int tdvp_launch(int op, int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a, int64_t b, int64_t c, int64_t d2,
                       const double* FL, const double* FR, const double* X, const double* M1, const double* M2, double* out, int m_shared,
                       bool host) {
    NEED_INIT();
    if (batch < 1 || Dl < 1 || d < 1 || Dr < 1 || a < 1 || b < 1 || c < 1 || d2 < 1 || !X || !out) return fail(TTN_ERR_ARG, "tdvp: bad argument");
    const int64_t lim = 1 << 20;
    if (Dl > 4096 || Dr > 4096 || d > 64 || d2 > 64 || a > 64 || b > 64 || c > 64 || Dl * Dr * d * d2 * std::max({a, b, c}) > (lim << 6))
        return fail(TTN_ERR_UNSUPPORTED, "tdvp: tensor too large");
    const long long es = cplx ? 2 : 1;
    long long nFL = 0, nFR = 0, nX = 0, nM1 = 0, nM2 = 0, nOut = 0, w1 = 0, w2 = 0;
    switch (op) {
    case 0: nFL = Dl * a * Dl; nFR = Dr * b * Dr; nX = Dl * d * Dr; nM1 = a * d * b * d; nOut = Dl * d * Dr; w1 = Dl * a * d * Dr; w2 = Dl * d * Dr * b; break;
    case 1: nFL = Dl * a * Dl; nFR = Dr * a * Dr; nX = Dl * Dr; nOut = Dl * Dr; w1 = Dl * a * Dr; w2 = 1; break;
    case 2: nFL = Dl * a * Dl; nX = Dl * d * Dr; nM1 = a * d * b * d; nOut = Dr * b * Dr; w1 = Dl * a * d * Dr; w2 = Dl * d * b * Dr; break;
    case 3: nFR = Dr * a * Dr; nX = Dl * d * Dr; nM1 = b * d * a * d; nOut = Dl * b * Dl; w1 = Dl * d * a * Dr; w2 = Dl * b * d * Dr; break;
    case 4: nFL = Dl * a * Dl; nFR = Dr * c * Dr; nX = Dl * d * d2 * Dr; nM1 = a * d * b * d; nM2 = b * d2 * c * d2; nOut = Dl * d * d2 * Dr;
            w1 = Dl * d * d2 * Dr * std::max(a, c); w2 = Dl * d * b * d2 * Dr; break;
    default: return fail(TTN_ERR_ARG, "tdvp: unknown contraction");
    }
    if ((nFL && !FL) || (nFR && !FR) || (nM1 && !M1) || (nM2 && !M2)) return fail(TTN_ERR_ARG, "tdvp: null tensor");
    const long long mb = m_shared ? 1 : batch;
    const size_t work_d = (size_t)(w1 + w2) * es * batch;
    const size_t stage_d = host ? (size_t)es * ((nFL + nFR + nX + nOut) * batch + (nM1 + nM2) * mb) : 0;
    int rc = scratch_take(sizeof(double) * (work_d + stage_d));
    if (rc) return rc;
    double* base = g_scratch.as<double>();
    TdvpArgs P;
    memset(&P, 0, sizeof(P));
    P.op = op; P.cplx = cplx;
    P.Dl = (int)Dl; P.d = (int)d; P.Dr = (int)Dr; P.a = (int)a; P.b = (int)b; P.c = (int)c; P.d2 = (int)d2;
    P.work = base; P.sWork = w1 + w2; P.w2off = w1;
    P.sFL = nFL; P.sFR = nFR; P.sX = nX; P.sOut = nOut; P.sM1 = m_shared ? 0 : nM1; P.sM2 = m_shared ? 0 : nM2;
    double* dout = out;
    if (host) {
        double* q = base + work_d;
        auto stage = [&](const double* src, long long n, long long cnt) -> const double* {
            if (!n) return nullptr;
            double* dst = q; q += (size_t)n * es * cnt;
            hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n * es * cnt, hipMemcpyHostToDevice, g_stream);
            return dst;
        };
        P.FL = stage(FL, nFL, batch); P.FR = stage(FR, nFR, batch); P.X = stage(X, nX, batch);
        P.M1 = stage(M1, nM1, mb); P.M2 = stage(M2, nM2, mb);
        dout = q;
    } else { P.FL = FL; P.FR = FR; P.X = X; P.M1 = M1; P.M2 = M2; }
    P.out = dout;
    hipLaunchKernelGGL(k_tdvp, dim3((unsigned)batch), dim3(TTN_WG), TDVP_LDS_BYTES, g_stream, P);
    HIPCHK(hipGetLastError());
    if (host) {
        HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)nOut * es * batch, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return TTN_OK;
}

int ttn_tdvp_apply_h1(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a, int64_t b, const double* FL, const double* AC,
                      const double* M, const double* FR, double* HAC, int m_shared) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return tdvp_launch(0, cplx, batch, Dl, d, Dr, a, b, 1, 1, FL, FR, AC, M, nullptr, HAC, m_shared, false);
}
int ttn_tdvp_apply_h0(int cplx, int64_t batch, int64_t Dl, int64_t Dr, int64_t a, const double* FL, const double* C, const double* FR, double* HC) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return tdvp_launch(1, cplx, batch, Dl, 1, Dr, a, 1, 1, 1, FL, FR, C, nullptr, nullptr, HC, 0, false);
}
int ttn_tdvp_update_left_env(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a_in, int64_t a_out, const double* A, const double* M,
                             const double* FL, double* FLnext, int m_shared) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return tdvp_launch(2, cplx, batch, Dl, d, Dr, a_in, a_out, 1, 1, FL, nullptr, A, M, nullptr, FLnext, m_shared, false);
}
int ttn_tdvp_update_right_env(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a_out, int64_t a_in, const double* A, const double* M,
                              const double* FR, double* FRprev, int m_shared) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return tdvp_launch(3, cplx, batch, Dl, d, Dr, a_in, a_out, 1, 1, nullptr, FR, A, M, nullptr, FRprev, m_shared, false);
}
int ttn_tdvp_apply_h2(int cplx, int64_t batch, int64_t Dl, int64_t d1, int64_t d2, int64_t Dr, int64_t a, int64_t b, int64_t c, const double* FL,
                      const double* AAC, const double* M1, const double* M2, const double* FR, double* HAAC, int m_shared) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return tdvp_launch(4, cplx, batch, Dl, d1, Dr, a, b, c, d2, FL, FR, AAC, M1, M2, HAAC, m_shared, false);
}
// ---- dense QR / SVD of one local matrix, real or complex, device pointers (csrc/ttn_densefact_kernels.h) ----
int ttn_dense_qr(int cplx, int64_t m, int64_t n, double* A, double* Q, double* R) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !Q || !R || m < 1 || n < 1) return fail(TTN_ERR_ARG, "ttn_dense_qr: bad argument");
    if (m > (1 << 20) || n > (1 << 20)) return fail(TTN_ERR_UNSUPPORTED, "ttn_dense_qr: matrix too large");
    const int64_t r = std::min(m, n);
    int rc = scratch_take(sizeof(double) * 2 * (size_t)r + 64);
    if (rc) return rc;
    if (cplx) hipLaunchKernelGGL(k_dense_qr<true>, dim3(1), dim3(TTN_DF_WG), 0, g_stream, (int)m, (int)n, A, Q, R, g_scratch.as<double>());
    else hipLaunchKernelGGL(k_dense_qr<false>, dim3(1), dim3(TTN_DF_WG), 0, g_stream, (int)m, (int)n, A, Q, R, g_scratch.as<double>());
    HIPCHK(hipGetLastError());
    return TTN_OK;
}
int ttn_dense_svd(int cplx, int64_t m, int64_t n, double* A, double* U, double* s, double* Vh) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !U || !s || !Vh || m < 1 || n < 1) return fail(TTN_ERR_ARG, "ttn_dense_svd: bad argument");
    if (m < n) return fail(TTN_ERR_ARG, "ttn_dense_svd: m >= n required (pass the conjugate transpose)");
    if (m > (1 << 20) || n > 4096) return fail(TTN_ERR_UNSUPPORTED, "ttn_dense_svd: matrix too large");
    const size_t w = cplx ? 2 : 1;
    const size_t vw = sizeof(double) * w * (size_t)n * n, dwb = sizeof(double) * ((size_t)n + (size_t)m);
    int rc = scratch_take(vw + dwb + sizeof(int) * ((size_t)n + 2) + 64);
    if (rc) return rc;
    double* Vw = g_scratch.as<double>();
    double* dw = Vw + w * (size_t)n * n;
    double* lw = dw + n;
    int* iw = reinterpret_cast<int*>(lw + m);
    if (cplx) hipLaunchKernelGGL(k_dense_svd<true>, dim3(1), dim3(TTN_DF_WG), 0, g_stream, (int)m, (int)n, A, U, s, Vh, Vw, dw, lw, iw, 60);
    else hipLaunchKernelGGL(k_dense_svd<false>, dim3(1), dim3(TTN_DF_WG), 0, g_stream, (int)m, (int)n, A, U, s, Vh, Vw, dw, lw, iw, 60);
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, iw + n, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (flag) return fail(TTN_ERR_NO_CONVERGENCE, "ttn_dense_svd: the Jacobi sweeps did not converge");
    return TTN_OK;
}

// ---- TT-cross (csrc/ttn_cross_kernels.h) --------------------------------------------------------------------------------------
static DevBuf g_cross_tab;        // core table of ttn_cross_eval
static DevBuf g_cross_info;       // status words of a ttn_cross_maxvol called without a device info
int ttn_cross_maxvol(int cplx, int64_t m, int64_t r, const double* A, double tol, int64_t maxiter, int64_t* piv, double* C, int64_t* dinfo,
                     int64_t* hinfo) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !piv || !C || m < 1 || r < 1 || maxiter < 0) return fail(TTN_ERR_ARG, "ttn_cross_maxvol: bad argument");
    if (m < r) return fail(TTN_ERR_ARG, "ttn_cross_maxvol: need m >= r");
    if (r > TTN_XV_MAX_R || m > TTN_XV_MAX_M) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_maxvol: need r <= 1024 and m <= 2^20");
    const size_t w = cplx ? 2 : 1, cbytes = sizeof(double) * w * (size_t)m * (size_t)r;
    const int use_lds = cbytes <= TTN_XV_LDS_C ? 1 : 0;
    const size_t wbytes = use_lds ? 0 : cbytes;
    int rc = scratch_take(wbytes + sizeof(int) * (size_t)m + 64);
    if (rc) return rc;
    if (!dinfo) {
        if ((rc = g_cross_info.ensure(sizeof(int64_t) * 2))) return rc;
        dinfo = g_cross_info.as<int64_t>();
    }
    double* Cw = g_scratch.as<double>();
    int* perm = reinterpret_cast<int*>(reinterpret_cast<char*>(g_scratch.p) + wbytes);
    const size_t lds = (use_lds ? cbytes : 0) + sizeof(double) * w * (size_t)r + sizeof(int) * (size_t)r;
    const int mi = (int)std::min<int64_t>(maxiter, 1 << 30);
    if (cplx)
        hipLaunchKernelGGL(k_cross_maxvol<true>, dim3(1), dim3(TTN_XV_WG), lds, g_stream, (int)m, (int)r, A, tol, mi, (long long*)piv, C, Cw, perm,
                           (long long*)dinfo, use_lds);
    else
        hipLaunchKernelGGL(k_cross_maxvol<false>, dim3(1), dim3(TTN_XV_WG), lds, g_stream, (int)m, (int)r, A, tol, mi, (long long*)piv, C, Cw, perm,
                           (long long*)dinfo, use_lds);
    HIPCHK(hipGetLastError());
    if (!hinfo) return TTN_OK;
    HIPCHK(hipMemcpyAsync(hinfo, dinfo, sizeof(int64_t) * 2, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (hinfo[0]) return fail(TTN_ERR_SINGULAR, "ttn_cross_maxvol: zero pivot (the matrix has rank < r)");
    return TTN_OK;
}

int ttn_cross_points(int cplx, int mode, int64_t N, int64_t site, int64_t n1, int64_t n2, int64_t rl, int64_t rr, const int64_t* L,
                     const int64_t* R, const int64_t* idx_in, int64_t P, const int64_t* doff, const double* dom, int64_t* idx_out, double* X) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!doff || N < 1 || P < 0 || mode < 0 || mode > 2 || (!idx_out && !X) || (X && !dom)) return fail(TTN_ERR_ARG, "ttn_cross_points: bad argument");
    if (mode == 2 && !idx_in) return fail(TTN_ERR_ARG, "ttn_cross_points: mode 2 needs an index matrix");
    if (mode != 2) {
        const int64_t last = mode == 0 ? N : N - 1;
        if (site < 1 || site > last || n1 < 1 || rl < 1 || rr < 1 || (mode == 1 && n2 < 1))
            return fail(TTN_ERR_ARG, "ttn_cross_points: bad site, size or rank");
        if ((site > 1 && !L) || (site < last && !R)) return fail(TTN_ERR_ARG, "ttn_cross_points: missing index set");
        const int64_t want = mode == 0 ? rl * n1 * rr : rl * n1 * n2 * rr;
        if (P != want) return fail(TTN_ERR_ARG, "ttn_cross_points: P differs from the size of the fibre / superblock");
    }
    if (P == 0) return TTN_OK;
    const long long total = (long long)P * N, blocks = (total + 255) / 256;
    if (cplx)
        hipLaunchKernelGGL(k_cross_points<true>, dim3((unsigned)blocks), dim3(256), 0, g_stream, mode, (long long)P, (int)N, (int)site, (long long)n1,
                           (long long)n2, (long long)rl, (long long)rr, (const long long*)L, (const long long*)R, (const long long*)idx_in,
                           (const long long*)doff, dom, (long long*)idx_out, X);
    else
        hipLaunchKernelGGL(k_cross_points<false>, dim3((unsigned)blocks), dim3(256), 0, g_stream, mode, (long long)P, (int)N, (int)site, (long long)n1,
                           (long long)n2, (long long)rl, (long long)rr, (const long long*)L, (const long long*)R, (const long long*)idx_in,
                           (const long long*)doff, dom, (long long*)idx_out, X);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_cross_eval(int cplx, int64_t N, int64_t P, const double* const* cores, const int64_t* dims, const int64_t* rks, const int64_t* idx,
                   const double* w, double* out, const double* yref, double tol, double* err) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!cores || !dims || !rks || !out || N < 1 || P < 1 || (!idx && !w) || (idx && w) || (w && P != 1) || (yref && !err))
        return fail(TTN_ERR_ARG, "ttn_cross_eval: bad argument (give idx, or w with P = 1)");
    if (rks[0] != 1 || rks[N] != 1) return fail(TTN_ERR_DIMS, "ttn_cross_eval: the end ranks must be 1");
    std::vector<long long> tab(4 * (size_t)N + 1);
    long long woff = 0;
    for (int64_t k = 0; k < N; ++k) {
        if (!cores[k] || dims[k] < 1 || rks[k] < 1) return fail(TTN_ERR_ARG, "ttn_cross_eval: bad core");
        tab[k] = (long long)reinterpret_cast<uintptr_t>(cores[k]);
        tab[N + k] = dims[k];
        tab[3 * N + 1 + k] = woff;
        woff += dims[k];
    }
    for (int64_t k = 0; k <= N; ++k) {
        if (rks[k] < 1 || rks[k] > TTN_XE_MAX_R) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_eval: ranks up to 1024");
        tab[2 * N + k] = rks[k];
    }
    int rc = g_cross_tab.ensure(sizeof(long long) * tab.size());
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(g_cross_tab.p, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice, g_stream));
    const long long* dtab = g_cross_tab.as<long long>();
    if (cplx) hipLaunchKernelGGL(k_cross_eval<true>, dim3((unsigned)P), dim3(64), 0, g_stream, (int)N, (long long)P, dtab, (const long long*)idx, w, w ? 1 : 0, out);
    else hipLaunchKernelGGL(k_cross_eval<false>, dim3((unsigned)P), dim3(64), 0, g_stream, (int)N, (long long)P, dtab, (const long long*)idx, w, w ? 1 : 0, out);
    HIPCHK(hipGetLastError());
    if (yref) {
        if (cplx) hipLaunchKernelGGL(k_cross_relerr<true>, dim3(1), dim3(TTN_XV_WG), 0, g_stream, (long long)P, yref, out, tol, err);
        else hipLaunchKernelGGL(k_cross_relerr<false>, dim3(1), dim3(TTN_XV_WG), 0, g_stream, (long long)P, yref, out, tol, err);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(g_stream));             // the table is a host local
    return TTN_OK;
}

// ---- MaxVol cross for a batch of functions (include/ttn_cross_batch.h, csrc/ttn_cross_batch_kernels.h) ----------------------------
static DevBuf g_xb_tab;           // core table of ttn_cross_batch_eval
static std::vector<long long> g_xb_tab_host;   // ttn_cross_batch_eval: the host copy of the core table, kept until its upload has completed
static hipEvent_t g_xb_tab_ev = nullptr;       // recorded after that upload; waited for before the host copy is written again
int ttn_cross_batch_points(int mode, int64_t A, int64_t N, int64_t site, int64_t n, int64_t rl, int64_t rr, const int64_t* L, const int64_t* R,
                           const int64_t* idx_in, int64_t P, const int64_t* doff, const double* dom, int64_t* idx_out, double* X) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!doff || A < 1 || N < 1 || P < 0 || (mode != 0 && mode != 2) || (!idx_out && !X) || (X && !dom))
        return fail(TTN_ERR_ARG, "ttn_cross_batch_points: bad argument");
    if (mode == 2 && !idx_in) return fail(TTN_ERR_ARG, "ttn_cross_batch_points: mode 2 needs an index matrix");
    if (mode == 0) {
        if (site < 1 || site > N || n < 1 || rl < 1 || rr < 1) return fail(TTN_ERR_ARG, "ttn_cross_batch_points: bad site, size or rank");
        if ((site > 1 && !L) || (site < N && !R)) return fail(TTN_ERR_ARG, "ttn_cross_batch_points: missing index set");
        if (P != rl * n * rr) return fail(TTN_ERR_ARG, "ttn_cross_batch_points: P differs from the size of the fibre");
    }
    if (A > TTN_XB_MAX_A) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_points: at most 65535 functions");
    if (P == 0) return TTN_OK;
    const long long total = (long long)P * N, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_points: too many points");
    hipLaunchKernelGGL(k_cross_batch_points, dim3((unsigned)blocks, (unsigned)A), dim3(256), 0, g_stream, mode, (long long)P, (int)N, (int)site,
                       (long long)n, (long long)rl, (long long)rr, (const long long*)L, (const long long*)R, (const long long*)idx_in,
                       (const long long*)doff, dom, (long long*)idx_out, X);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_cross_batch_site(int64_t A, int dir, int64_t N, int64_t site, int64_t n, int64_t rl, int64_t rr, const double* V, double tol,
                         int64_t maxiter, const int64_t* set_in, int64_t* set_out, double* core, int64_t* piv, int64_t* info) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!V || !set_out || !core || !piv || !info || A < 1 || N < 2 || (dir != 0 && dir != 1) || n < 1 || rl < 1 || rr < 1 || maxiter < 0)
        return fail(TTN_ERR_ARG, "ttn_cross_batch_site: bad argument");
    if (dir == 0 ? (site < 1 || site > N - 1) : (site < 2 || site > N)) return fail(TTN_ERR_ARG, "ttn_cross_batch_site: bad site for this direction");
    const int64_t nin = dir == 0 ? site - 1 : N - site;
    if (nin > 0 && !set_in) return fail(TTN_ERR_ARG, "ttn_cross_batch_site: missing index set");
    if (nin == 0 && (dir == 0 ? rl : rr) != 1) return fail(TTN_ERR_ARG, "ttn_cross_batch_site: the end rank must be 1");
    if (rl > TTN_XV_MAX_M || rr > TTN_XV_MAX_M || n > TTN_XV_MAX_M) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_site: need r <= 1024 and m <= 2^20");
    const int64_t m = dir == 0 ? rl * n : n * rr, r = dir == 0 ? rr : rl;
    if (m < r) return fail(TTN_ERR_ARG, "ttn_cross_batch_site: need m >= r");
    if (r > TTN_XV_MAX_R || m > TTN_XV_MAX_M) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_site: need r <= 1024 and m <= 2^20");
    if (A > TTN_XB_MAX_A) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_site: at most 65535 functions");
    const size_t sz = (size_t)m * (size_t)r;
    const int use_lds = 2 * sizeof(double) * sz <= TTN_XB_LDS_MAT ? 1 : 0;
    const size_t stride = (use_lds ? 0 : 2 * sz) + (dir == 0 ? 0 : sz) + ((size_t)m + 1) / 2;       // doubles per function
    int rc = scratch_take(sizeof(double) * stride * (size_t)A + 64);
    if (rc) return rc;
    const size_t lds = (use_lds ? 2 * sizeof(double) * sz : 0) + TTN_XB_LDS_SMALL(r);
    const int mi = (int)std::min<int64_t>(maxiter, 1 << 30);
    hipLaunchKernelGGL(k_cross_batch_site, dim3((unsigned)A), dim3(TTN_XB_WG), lds, g_stream, dir, (int)n, (int)rl, (int)rr, (int)nin, V, tol, mi,
                       (const long long*)set_in, (long long*)set_out, core, (long long*)piv, (long long*)info, g_scratch.as<double>(),
                       (long long)stride, use_lds);
    HIPCHK(hipGetLastError());
    return TTN_OK;
}

int ttn_cross_batch_eval(int64_t A, int64_t N, int64_t P, const double* const* cores, const int64_t* dims, const int64_t* rks,
                         const int64_t* idx, const double* w, double* out, const double* yref, double tol, double* err) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!cores || !dims || !rks || !out || A < 1 || N < 1 || P < 1 || (!idx && !w) || (idx && w) || (w && P != 1) || (yref && !err))
        return fail(TTN_ERR_ARG, "ttn_cross_batch_eval: bad argument (give idx, or w with P = 1)");
    if (rks[0] != 1 || rks[N] != 1) return fail(TTN_ERR_DIMS, "ttn_cross_batch_eval: the end ranks must be 1");
    for (int64_t k = 0; k < N; ++k)
        if (!cores[k] || dims[k] < 1) return fail(TTN_ERR_ARG, "ttn_cross_batch_eval: bad core");
    for (int64_t k = 0; k <= N; ++k)
        if (rks[k] < 1 || rks[k] > TTN_XE_MAX_R) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_eval: ranks up to 1024");
    if (A > TTN_XB_MAX_A || P > 0x7fffffffLL) return fail(TTN_ERR_UNSUPPORTED, "ttn_cross_batch_eval: at most 65535 functions");
    // the table travels from a host copy that stays untouched until the upload has completed: no wait on the stream here
    if (!g_xb_tab_ev) HIPCHK(hipEventCreateWithFlags(&g_xb_tab_ev, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(g_xb_tab_ev));
    g_xb_tab_host.assign(4 * (size_t)N + 1, 0);
    long long woff = 0;
    for (int64_t k = 0; k < N; ++k) {
        g_xb_tab_host[k] = (long long)reinterpret_cast<uintptr_t>(cores[k]);
        g_xb_tab_host[N + k] = dims[k];
        g_xb_tab_host[3 * N + 1 + k] = woff;
        woff += dims[k];
    }
    for (int64_t k = 0; k <= N; ++k) g_xb_tab_host[2 * N + k] = rks[k];
    const size_t tbytes = sizeof(long long) * g_xb_tab_host.size();
    int rc = g_xb_tab.ensure(tbytes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(g_xb_tab.p, g_xb_tab_host.data(), tbytes, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipEventRecord(g_xb_tab_ev, g_stream));
    hipLaunchKernelGGL(k_cross_batch_eval, dim3((unsigned)P, (unsigned)A), dim3(64), 0, g_stream, (int)N, (long long)P, g_xb_tab.as<long long>(),
                       (const long long*)idx, w, w ? 1 : 0, out);
    HIPCHK(hipGetLastError());
    if (yref) {
        hipLaunchKernelGGL(k_cross_batch_relerr, dim3((unsigned)A), dim3(TTN_XB_WG), 0, g_stream, (long long)P, yref, out, tol, err);
        HIPCHK(hipGetLastError());
    }
    return TTN_OK;
}

// host-array forms (what a `ccall` from tdvp1sweep! / tdvp2sweep! binds): op = 0 applyH1, 1 applyH0, 2 update_left_env,
// 3 update_right_env, 4 applyH2; dims = {Dl, d (d1), Dr, a, b, c, d2} with the meaning of the device forms above
int ttn_tdvp_contract_f64(int op, int cplx, int64_t batch, const int64_t* dims7, const double* FL, const double* FR, const double* X, const double* M1,
                          const double* M2, double* out, int m_shared) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!dims7) return fail(TTN_ERR_ARG, "tdvp: null dims");
    return tdvp_launch(op, cplx, batch, dims7[0], dims7[1], dims7[2], dims7[3], dims7[4], dims7[5], dims7[6], FL, FR, X, M1, M2, out, m_shared, true);
}

// ---- stateless entry points on host arrays ----------------------------------------------------------------------------------------
// Each one is: operands onto the device (host_tt / host_tto), the handle call, the result back (host_result).  The _f64 and _c64
// exports of an operation share one body that takes the element type of every operand (el: 1 Float64, 2 ComplexF64 as interleaved
// (re, im) doubles).
namespace {
int auto_init() {
    if (g_init) return TTN_OK;
    return ttn_init(0);
}
// a one-train handle of capacity `cap`; with `cores` it holds that train (ranks rks, gauge flags ot or zeros)
int host_tt(OwnedTT& t, int el, int64_t d, const int64_t* dims, const int64_t* cap, const double* const* cores = nullptr, const int64_t* rks = nullptr,
            const int64_t* ot = nullptr) {
    const int rc = tt_create_impl(d, dims, cap, 1, &t.h, el);
    if (rc || !cores) return rc;
    return ttn_tt_upload(t.h, 0, cores, rks, ot);
}
int host_tto(OwnedTTO& A, int el, int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores) {
    return tto_create_impl(d, dims, rks, cores, &A.h, el);
}
// the result of a stateless call: with `status`, a failure the dense kernels recorded on h is the call's error; then the ranks and
// gauge flags that are asked for, and the cores
int host_result(ttn_tt_t h, bool status, int64_t* rks, int64_t* ot, double* const* cores) {
    int rc;
    if (status && (rc = ttn_compress_status(h, nullptr))) return rc;
    if ((rks || ot) && (rc = ttn_tt_ranks(h, 0, rks, ot))) return rc;
    return ttn_tt_download(h, 0, cores);
}

int apply_host(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
               const int64_t* X_rks, double* const* Y_cores, int a_el, int x_el, int y_el) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !A_cores || !A_rks || !X_cores || !X_rks || !Y_cores || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    OwnedTTO A; OwnedTT x, y;
    if ((rc = host_tto(A, a_el, d, dims, A_rks, A_cores))) return rc;
    if ((rc = host_tt(x, x_el, d, dims, X_rks, X_cores, X_rks))) return rc;
    std::vector<int64_t> yr(d + 1);
    for (int64_t m = 0; m <= d; ++m) yr[m] = A_rks[m] * X_rks[m];
    if ((rc = host_tt(y, y_el, d, dims, yr.data()))) return rc;
    if ((rc = ttn_apply(A.h, x.h, y.h))) return rc;
    return host_result(y.h, false, nullptr, nullptr, Y_cores);
}

int dot_host(int el, int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* B_cores,
             const int64_t* B_rks, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !A_cores || !A_rks || !B_cores || !B_rks || !out || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    OwnedTT a, b;
    if ((rc = host_tt(a, el, d, dims, A_rks, A_cores, A_rks))) return rc;
    if ((rc = host_tt(b, el, d, dims, B_rks, B_cores, B_rks))) return rc;
    return ttn_dot(a.h, b.h, out);
}

// z = x + y (sum) or the Hadamard product: the two differ in the ranks of z and in the handle call
int binary_host(bool sum, int el, int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, const double* const* Y_cores,
                const int64_t* Y_rks, double* const* Z_cores) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !X_cores || !X_rks || !Y_cores || !Y_rks || !Z_cores || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    OwnedTT x, y, z;
    std::vector<int64_t> zr(d + 1);
    for (int64_t m = 0; m <= d; ++m) zr[m] = !sum ? X_rks[m] * Y_rks[m] : (m == 0 || m == d) ? 1 : X_rks[m] + Y_rks[m];
    if ((rc = host_tt(x, el, d, dims, X_rks, X_cores, X_rks))) return rc;
    if ((rc = host_tt(y, el, d, dims, Y_rks, Y_cores, Y_rks))) return rc;
    if ((rc = host_tt(z, el, d, dims, zr.data()))) return rc;
    if ((rc = sum ? ttn_add(x.h, y.h, z.h) : ttn_hadamard(x.h, y.h, z.h))) return rc;
    return host_result(z.h, false, nullptr, nullptr, Z_cores);
}

int scale_host(int el, int64_t d, const int64_t* dims, double re, double im, const double* const* X_cores, const int64_t* X_rks,
               const int64_t* X_ot, double* const* Y_cores, int64_t* Y_ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !X_cores || !X_rks || !Y_cores || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    OwnedTT x, y;
    if ((rc = host_tt(x, el, d, dims, X_rks, X_cores, X_rks, X_ot))) return rc;
    if ((rc = host_tt(y, el, d, dims, X_rks))) return rc;
    if ((rc = el == 2 ? ttn_scale_c64(re, im, x.h, y.h) : ttn_scale(re, x.h, y.h))) return rc;
    return host_result(y.h, false, nullptr, Y_ot, Y_cores);
}

// tt_compress! (k = 0) or one _tt_bond_truncate! (k > 0) in place on the caller's buffers; the caller has held the lock and checked
// sweeps / k, which need no device
int compress_host(int el, int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t k, int64_t max_bond, double truncerr,
                  int64_t sweeps) {
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !cores || !rks || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    OwnedTT x;
    std::vector<int64_t> need, fin;
    long long pm, qm;
    rank_bounds((int)d, dims, rks, max_bond, sweeps, k, need, fin, pm, qm);
    if ((rc = host_tt(x, el, d, dims, need.data(), cores, rks))) return rc;
    if (k > 0) rc = ttn_bond_truncate(x.h, k, max_bond, truncerr);
    else rc = ttn_compress(x.h, max_bond, truncerr, sweeps);
    if (rc) return rc;
    return host_result(x.h, true, rks, nullptr, cores);
}

// The ranks yr = A_rks .* X_rks of A * x and what rounding it can reach: need[m] >= yr[m] covers every rank bond m takes during
// tt_compress!(A * x, max_bond; sweeps), fin[m] bounds it afterwards.
void product_rank_bounds(int64_t d, const int64_t* dims, const int64_t* A_rks, const int64_t* X_rks, int64_t max_bond, int64_t sweeps,
                         std::vector<int64_t>& need, std::vector<int64_t>& fin) {
    std::vector<int64_t> yr(d + 1);
    for (int64_t m = 0; m <= d; ++m) yr[m] = A_rks[m] * X_rks[m];
    long long pm, qm;
    rank_bounds((int)d, dims, yr.data(), max_bond, sweeps, 0, need, fin, pm, qm);
    for (int64_t m = 0; m <= d; ++m) need[m] = std::max<int64_t>(need[m], yr[m]);
}

int apply_compress_host(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                        const int64_t* X_rks, double* const* Y_cores, int64_t* Y_rks, int64_t max_bond, double truncerr, int64_t sweeps,
                        int a_el, int x_el, int y_el) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !A_cores || !A_rks || !X_cores || !X_rks || !Y_cores || !Y_rks || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    OwnedTTO A; OwnedTT x, y;
    if ((rc = host_tto(A, a_el, d, dims, A_rks, A_cores))) return rc;
    if ((rc = host_tt(x, x_el, d, dims, X_rks, X_cores, X_rks))) return rc;
    std::vector<int64_t> need, fin;
    product_rank_bounds(d, dims, A_rks, X_rks, max_bond, sweeps, need, fin);
    if ((rc = host_tt(y, y_el, d, dims, need.data()))) return rc;
    if ((rc = ttn_apply_compress(A.h, x.h, y.h, max_bond, truncerr, sweeps))) return rc;
    return host_result(y.h, true, Y_rks, nullptr, Y_cores);
}
}  // namespace

int ttn_apply_f64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks,
                  const double* const* X_cores, const int64_t* X_rks, double* const* Y_cores) {
    return apply_host(d, dims, A_cores, A_rks, X_cores, X_rks, Y_cores, 1, 1, 1);
}
// the rectangular form for one train: Y_cores[k] sized out_dims[k] * yr[k] * yr[k + 1], yr[b] = A_rks[b] * X_rks[c(b)]
int ttn_apply_rect_f64(int64_t M, const int64_t* out_dims, const int64_t* in_dims, const double* const* A_cores, const int64_t* A_rks,
                       const double* const* X_cores, const int64_t* X_rks, double* const* Y_cores) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!out_dims || !in_dims || !A_cores || !A_rks || !X_cores || !X_rks || !Y_cores || M < 2) return fail(TTN_ERR_ARG, "bad argument");
    OwnedRTTO A; OwnedTT x, y;
    if ((rc = ttn_rtto_create(M, out_dims, in_dims, A_rks, A_cores, &A.h))) return rc;
    if (A.h->singles.size() != 1) return fail(TTN_ERR_DIMS, "Rectangular TToperator must have exactly one singleton input site");
    const int s = A.h->singles[0];
    std::vector<int64_t> xd(M - 1), yr(M + 1);
    for (int64_t k = 0; k + 1 < M; ++k) xd[k] = in_dims[k < s ? k : k + 1];
    for (int64_t m = 0; m <= M; ++m) yr[m] = A_rks[m] * X_rks[m > s ? m - 1 : m];
    if ((rc = host_tt(x, 1, M - 1, xd.data(), X_rks, X_cores, X_rks))) return rc;
    if ((rc = host_tt(y, 1, M, out_dims, yr.data()))) return rc;
    if ((rc = ttn_apply_rect(A.h, x.h, y.h))) return rc;
    return host_result(y.h, false, nullptr, nullptr, Y_cores);
}
// a real operator or train stays real on the device; the result is complex
int ttn_apply_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                  const int64_t* X_rks, double* const* Y_cores, int a_cplx, int x_cplx) {
    return apply_host(d, dims, A_cores, A_rks, X_cores, X_rks, Y_cores, a_cplx ? 2 : 1, x_cplx ? 2 : 1, 2);
}

int ttn_dot_f64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks,
                const double* const* B_cores, const int64_t* B_rks, double* out) {
    return dot_host(1, d, dims, A_cores, A_rks, B_cores, B_rks, out);
}
int ttn_dot_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* B_cores,
                const int64_t* B_rks, double* out) {
    return dot_host(2, d, dims, A_cores, A_rks, B_cores, B_rks, out);
}

int ttn_hadamard_f64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks,
                     const double* const* Y_cores, const int64_t* Y_rks, double* const* Z_cores) {
    return binary_host(false, 1, d, dims, X_cores, X_rks, Y_cores, Y_rks, Z_cores);
}
int ttn_hadamard_c64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, const double* const* Y_cores,
                     const int64_t* Y_rks, double* const* Z_cores) {
    return binary_host(false, 2, d, dims, X_cores, X_rks, Y_cores, Y_rks, Z_cores);
}

int ttn_add_f64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks,
                const double* const* Y_cores, const int64_t* Y_rks, double* const* Z_cores) {
    return binary_host(true, 1, d, dims, X_cores, X_rks, Y_cores, Y_rks, Z_cores);
}
int ttn_add_c64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, const double* const* Y_cores,
                const int64_t* Y_rks, double* const* Z_cores) {
    return binary_host(true, 2, d, dims, X_cores, X_rks, Y_cores, Y_rks, Z_cores);
}

int ttn_scale_f64(int64_t d, const int64_t* dims, double a, const double* const* X_cores, const int64_t* X_rks,
                  const int64_t* X_ot, double* const* Y_cores, int64_t* Y_ot) {
    return scale_host(1, d, dims, a, 0.0, X_cores, X_rks, X_ot, Y_cores, Y_ot);
}
int ttn_scale_host_c64(int64_t d, const int64_t* dims, double re, double im, const double* const* X_cores, const int64_t* X_rks,
                       const int64_t* X_ot, double* const* Y_cores, int64_t* Y_ot) {
    return scale_host(2, d, dims, re, im, X_cores, X_rks, X_ot, Y_cores, Y_ot);
}

int ttn_orthogonalize_f64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, int64_t center,
                          double* const* Y_cores, int64_t* Y_rks, int64_t* Y_ot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = auto_init(); if (rc) return rc;
    if (!dims || !X_cores || !X_rks || !Y_cores || !Y_rks || !Y_ot || d < 1) return fail(TTN_ERR_ARG, "bad argument");
    if (center < 1 || center > d) return fail(TTN_ERR_CENTER, "Impossible orthogonalization");
    OwnedTT x, y;
    if ((rc = host_tt(x, 1, d, dims, X_rks, X_cores, X_rks))) return rc;
    if ((rc = host_tt(y, 1, d, dims, X_rks))) return rc;
    if ((rc = ttn_orthogonalize(x.h, center, y.h))) return rc;
    return host_result(y.h, false, Y_rks, Y_ot, Y_cores);
}

int ttn_compress_f64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t max_bond, double truncerr,
                     int64_t sweeps) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    return compress_host(1, d, dims, cores, rks, 0, max_bond, truncerr, sweeps);
}
int ttn_compress_c64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t max_bond, double truncerr, int64_t sweeps) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    return compress_host(2, d, dims, cores, rks, 0, max_bond, truncerr, sweeps);
}

int ttn_bond_truncate_f64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t k, int64_t max_bond,
                          double truncerr) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (k < 1 || k >= d) return fail(TTN_ERR_BOND_INDEX, "k must be in 1:(N-1)");
    return compress_host(1, d, dims, cores, rks, k, max_bond, truncerr, 1);
}
int ttn_bond_truncate_c64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t k, int64_t max_bond, double truncerr) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (k < 1 || k >= d) return fail(TTN_ERR_BOND_INDEX, "k must be in 1:(N-1)");
    return compress_host(2, d, dims, cores, rks, k, max_bond, truncerr, 1);
}

// The Krylov operator of the reference in ONE stateless call: op = x -> tt_compress!(A * x, max_bond) (src/solvers/euler.jl:55).  A * x
// is never materialised (fused apply, k_compress builds the merged matrices from x and A) — neither in HBM nor over PCIe: the host
// hands over A and x, and receives the compressed train.  Y_cores[k] sized n_k * cap_k * cap_{k+1} with cap = min(A_rks .* X_rks,
// max_bond-capped bounds) as ttn_apply_compress_rank_bound returns them; Y_rks receives the ranks.  (ComplexF64: apply, then round.)
int ttn_apply_compress_rank_bound(int64_t d, const int64_t* dims, const int64_t* A_rks, const int64_t* X_rks, int64_t max_bond, int64_t sweeps,
                                  int64_t* cap) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!dims || !A_rks || !X_rks || !cap || d < 1 || max_bond < 1 || sweeps < 1) return fail(TTN_ERR_ARG, "bad argument");
    std::vector<int64_t> need, fin;
    product_rank_bounds(d, dims, A_rks, X_rks, max_bond, sweeps, need, fin);
    for (int64_t m = 0; m <= d; ++m) cap[m] = fin[m];
    return TTN_OK;
}
int ttn_apply_compress_f64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                           const int64_t* X_rks, double* const* Y_cores, int64_t* Y_rks, int64_t max_bond, double truncerr, int64_t sweeps) {
    return apply_compress_host(d, dims, A_cores, A_rks, X_cores, X_rks, Y_cores, Y_rks, max_bond, truncerr, sweeps, 1, 1, 1);
}
int ttn_apply_compress_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                           const int64_t* X_rks, double* const* Y_cores, int64_t* Y_rks, int64_t max_bond, double truncerr, int64_t sweeps,
                           int a_cplx, int x_cplx) {
    return apply_compress_host(d, dims, A_cores, A_rks, X_cores, X_rks, Y_cores, Y_rks, max_bond, truncerr, sweeps, a_cplx ? 2 : 1, x_cplx ? 2 : 1, 2);
}

// ---- als_eigsolve / als_gen_eigsolv (csrc/ttn_als_eig_kernels.h) ---------------------------------------------------------------
static DevBuf g_als_tab;          // slot table and stage ranks of the one-site eigensolvers
// The host walks the stages of the schedule (als.jl:284-300, :370-397): k_als_eig runs a stage's full sweeps at fixed ranks, writing
// its part of the history; between stages k_increase_ranks pads x into a temporary handle of x's capacity at the ranks
// r_and_d_to_rks(fill(rmax)) and ttn_orthogonalize brings it back into x (it does not allow aliasing).  The environments of every
// stage are rebuilt from the re-orthogonalised train — for als_gen_eigsolv too, where the reference zero-pads the stale right
// environments instead (als.jl:379-396), which leaves the first solves of a new stage with a singular metric.
static int als_eig_impl(int gen, ttn_tto_t A, ttn_tto_t S, ttn_tt_t x0, ttn_tt_t x, int64_t n_stages, const int64_t* sweep_schedule,
                        const int64_t* rmax_schedule, const double* noise_schedule, int64_t seed, int it_solver, int64_t maxiter,
                        double linsolv_tol, int64_t itslv_thresh, int64_t hist_len, double* E_out) {
    const char* who = gen ? "als_gen_eigsolv" : "als_eigsolve";
    auto err = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
    NEED_INIT();
    F64_ONLY("one-site eigensolver", {x0, x}, {A, S});
    if (!A || !x0 || !x || (gen && !S)) return err(TTN_ERR_ARG, "null handle");
    if (!rmax_schedule || (hist_len > 0 && !E_out)) return err(TTN_ERR_ARG, "null schedule / history buffer");
    if (!same_dims(A->dims, x0->dims) || !same_dims(x0->dims, x->dims) || (gen && !same_dims(S->dims, x0->dims)))
        return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != x0->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    const int d = x0->d;
    if (d < 2) return err(TTN_ERR_UNSUPPORTED, "needs at least two sites");
    if (maxiter < 1 || !(linsolv_tol >= 0.0) || itslv_thresh < 0) return err(TTN_ERR_ARG, "bad maxiter / linsolv_tol / itslv_thresh");
    std::vector<int64_t> plan;
    int rc = sweep_plan(who, TTN_ERR_ARG, n_stages, sweep_schedule, rmax_schedule, plan);
    if (rc) return rc;
    const int64_t per = 2 * (int64_t)(d - 1);
    if (hist_len != per * (int64_t)plan.size()) return err(TTN_ERR_ARG, "hist_len differs from ttn_eigsolve_history_len");
    if (noise_schedule)
        for (int64_t j = 0; j < n_stages; ++j) if (!(noise_schedule[j] >= 0.0 || noise_schedule[j] < 0.0)) return err(TTN_ERR_ARG, "noise_schedule is not finite");
    // ---- every check before anything is launched ----
    const std::vector<int64_t>& r0 = x0->bound;
    {
        std::vector<int64_t> capped(d + 1);
        ttn_r_and_d_to_rks(d, x0->dims.data(), d + 1, r0.data(), 1024, capped.data());
        for (int k = 0; k <= d; ++k) if (capped[k] != r0[k]) return err(TTN_ERR_UNSUPPORTED, "the start ranks exceed what orthogonalize keeps");
        for (int i = 0; i < d; ++i)
            if (x0->dims[i] * r0[i] < r0[i + 1] || x0->dims[i] * r0[i + 1] < r0[i]) return err(TTN_ERR_UNSUPPORTED, "a core is too flat for the QR core moves");
    }
    std::vector<std::vector<int64_t>> stage_rks(n_stages);            // ranks of every stage after its rank increase (stage 0: the start)
    stage_rks[0] = r0;
    for (int64_t j = 1; j < n_stages; ++j) {
        const int64_t top = *std::max_element(stage_rks[j - 1].begin(), stage_rks[j - 1].end());
        if (rmax_schedule[j] <= top) return err(TTN_ERR_ARG, "New bond dimension too low (a stage's rmax must exceed the current maximum rank)");
        std::vector<int64_t> fill(d + 1, rmax_schedule[j]);
        fill[0] = 1; fill[d] = 1;
        stage_rks[j].assign(d + 1, 1);
        ttn_r_and_d_to_rks(d, x0->dims.data(), d + 1, fill.data(), rmax_schedule[j], stage_rks[j].data());
    }
    std::vector<int64_t> rl(d + 1, 1);                                 // the largest rank any stage holds: the slot sizes
    for (const auto& v : stage_rks) for (int k = 0; k <= d; ++k) rl[k] = std::max(rl[k], v[k]);
    for (int k = 0; k <= d; ++k) if (x->cap[k] < rl[k]) return err(TTN_ERR_CAPACITY, "the rank capacity of x is below the ranks of a stage");
    const std::vector<int64_t>& RA = A->rks;
    const std::vector<int64_t>& RS = gen ? S->rks : A->rks;
    long long cur = 0, Nmax = 1, mmax = 1, cmax = 1, t1 = 1, t2 = 1, Rzmax = 1;
    std::vector<long long> off(4 * d, 0);
    for (int i = 0; i < d; ++i) {
        const long long n = x0->dims[i], a = rl[i], c = rl[i + 1];
        off[i] = cur; cur += n * a * n * a * RA[i + 1];
        if (gen) { off[d + i] = cur; cur += n * a * n * a * RS[i + 1]; }
        off[2 * d + i] = cur; cur += RA[i + 1] * c * c;
        if (gen) { off[3 * d + i] = cur; cur += RS[i + 1] * c * c; }
        Nmax = std::max(Nmax, n * a * c);
        mmax = std::max(mmax, std::max(n * a, n * c));
        cmax = std::max(cmax, std::max(a, c));
        for (const std::vector<int64_t>* R : {&RA, &RS}) {
            const long long Rl = (*R)[i], Rr = (*R)[i + 1];
            t1 = std::max(t1, n * a * c * std::max<long long>(Rr, 1));
            t2 = std::max(t2, std::max(c * c * Rr, n * c * Rl * a));
            Rzmax = std::max(Rzmax, Rr);
        }
    }
    if (Nmax > 65536) return err(TTN_ERR_UNSUPPORTED, "local problems above 65 536 unknowns (n_i r_{i-1} r_i) are not supported");
    // branch rule: standard dense unless N > 2048 or (it_solver and N > itslv_thresh) (als.jl:74); generalized dense only when !it_solver
    // and N <= min(itslv_thresh, 2048) (als.jl:95)
    const long long dense_cap = TTN_DENSE_LOCAL_MAX_ALS;
    const long long it_above = gen ? (it_solver ? 0 : std::min<long long>(itslv_thresh, dense_cap))
                                   : (it_solver ? std::min<long long>(itslv_thresh, dense_cap) : dense_cap);
    const bool need_it = Nmax > it_above;
    const long long Kdim = std::min<long long>(Nmax, it_above);
    AlsEigArgs Rg;
    memset(&Rg, 0, sizeof(Rg));
    Rg.offK = cur; cur += Kdim * Kdim;
    Rg.offK2 = cur; if (gen) cur += Kdim * Kdim;
    Rg.offEig = cur; cur += 8 + 8 * Kdim;
    Rg.offPb = cur; cur += Nmax;
    Rg.offIt = cur;
    if (need_it) { Rg.it_nmax = Nmax; cur += gen ? (9 + Rzmax) * Nmax + 64 : (TTN_LZ_M + 1 + TTN_LZ_KEEP + Rzmax) * Nmax + 5000; }
    Rg.offT1 = cur; cur += t1;
    Rg.offT2 = cur; cur += t2;
    Rg.offTm = cur; cur += mmax * cmax;
    Rg.offQb = cur; cur += mmax * cmax;
    Rg.offRb = cur; cur += cmax * cmax;
    Rg.offVb = cur; cur += QR_NB * mmax;
    Rg.offWb = cur; cur += QR_NB * mmax;
    Rg.offTst = cur; cur += ((cmax + QR_NB - 1) / QR_NB) * QR_NB * QR_NB + 64;
    const long long per_train = cur;
    const int batch = x->batch;
    const size_t need = sizeof(double) * (size_t)per_train * batch;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        if (need > g_scratch.bytes && need - g_scratch.bytes > free_b)
            return err(TTN_ERR_CAPACITY, "the workspace of this capacity and batch (environments, dense local matrices, iterative basis) does not fit in device memory");
    }
    // ---- the solve ----
    rc = ttn_orthogonalize(x0, 1, x);                                  // als.jl:264, :350
    if (rc) return rc;
    const size_t hn = (size_t)batch * (size_t)std::max<int64_t>(hist_len, 1);
    if ((rc = g_hist_E.ensure(sizeof(double) * hn)) || (rc = g_lz_iters.ensure(sizeof(int) * batch)) || (rc = g_lz_res.ensure(sizeof(double) * batch)) ||
        (rc = g_als_tab.ensure(sizeof(long long) * (4 * (size_t)d + d + 1))))
        return rc;
    HIPCHK(hipMemsetAsync(g_lz_iters.p, 0, sizeof(int) * batch, g_stream));
    HIPCHK(hipMemsetAsync(g_lz_res.p, 0, sizeof(double) * batch, g_stream));
    HIPCHK(hipMemsetAsync(x->d_status, 0, sizeof(int) * batch, g_stream));
    long long* d_off = g_als_tab.as<long long>();
    long long* d_rn = d_off + 4 * d;
    HIPCHK(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));                            // off is a local
    Rg.A = A->dev(); Rg.S = gen ? S->dev() : A->dev();
    Rg.gen = gen;
    Rg.off = d_off;
    Rg.it_above = (int)it_above;
    Rg.lz_maxrestart = (int)std::min<int64_t>(maxiter, 1 << 30);
    Rg.lz_tol = linsolv_tol;
    Rg.status = x->d_status;
    Rg.hist_E = g_hist_E.as<double>(); Rg.hist_len = (int)hist_len;
    Rg.it_count = g_lz_iters.as<int>(); Rg.it_res = g_lz_res.as<double>();
    OwnedTT tmp;
    if (n_stages > 1 && (rc = ttn_tt_create(d, x->dims.data(), x->cap.data(), batch, &tmp.h))) return rc;
    int64_t hoff = 0;
    for (int64_t j = 0; j < n_stages; ++j) {
        if (j > 0) {                                                   // increase_ranks -> orthogonalize (als.jl:291-292, :377-378)
            if ((rc = scratch_take(need))) return rc;                  // nothing survives: k_increase_ranks only writes Tm .. Tst before it reads them
            HIPCHK(hipMemcpyAsync(d_rn, stage_rks[j].data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
            IncArgs Ia;
            memset(&Ia, 0, sizeof(Ia));
            Ia.x = x->dev(); Ia.y = tmp.h->dev(); Ia.rn = d_rn;
            Ia.noise = noise_schedule ? noise_schedule[j] : 0.0;
            Ia.seed = seed;
            Ia.scratch = g_scratch.as<double>(); Ia.scratch_stride = per_train;
            Ia.offTm = Rg.offTm; Ia.offQb = Rg.offQb; Ia.offRb = Rg.offRb; Ia.offVb = Rg.offVb; Ia.offWb = Rg.offWb; Ia.offTst = Rg.offTst;
            hipLaunchKernelGGL(k_increase_ranks, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Ia);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(g_stream));                    // stage_rks is the host's until the copy is done
            tmp.h->bound = stage_rks[j];
            std::fill(tmp.h->ot.begin(), tmp.h->ot.end(), 0);
            if ((rc = ttn_orthogonalize(tmp.h, 1, x))) return rc;
        }
        const int64_t nsw = sweep_schedule[j] - (j ? sweep_schedule[j - 1] : 1);
        if (nsw > 0) {
            // ttn_orthogonalize shares the workspace, so it is taken again every stage — and nothing of the stage before survives:
            // k_als_eig rebuilds G_1 and every H_i from the cores first thing (init_env), whatever the workspace holds
            if ((rc = scratch_take(need))) return rc;
            Rg.x = x->dev();
            Rg.scratch = g_scratch.as<double>(); Rg.scratch_stride = per_train;
            Rg.nsweeps = (int)nsw;
            Rg.hist_off = (int)hoff;
            hipLaunchKernelGGL(k_als_eig, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Rg);
            HIPCHK(hipGetLastError());
            hoff += nsw * per;
        }
    }
    g_lz_iters_host.assign(batch, 0);
    g_lz_res_host.assign(batch, 0.0);
    if (hist_len > 0) HIPCHK(hipMemcpyAsync(E_out, g_hist_E.p, sizeof(double) * (size_t)batch * hist_len, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(g_lz_iters_host.data(), g_lz_iters.p, sizeof(int) * batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(g_lz_res_host.data(), g_lz_res.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g_stream));
    unsigned seen = 0;
    rc = take_status(x, seen);                                         // synchronises the copies above too
    if (rc) return rc;
    // gauge flags: after a backward half sweep x_1 carries the norm, the others are right-orthogonal (als.jl:112-118)
    if (!plan.empty())
        for (int bb = 0; bb < batch; ++bb)
            for (int k = 0; k < d; ++k) x->ot[(size_t)bb * d + k] = (k == 0) ? 0 : 1;
    return status_error(seen, who);
}

int ttn_als_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                     const double* noise_schedule, int64_t seed, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                     int64_t hist_len, double* E) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_als_eigsolve")) return rb;
    return als_eig_impl(0, A, nullptr, x0, x, n_stages, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter, linsolv_tol,
                        itslv_thresh, hist_len, E);
}

int ttn_als_gen_eigsolve(ttn_tto_t A, ttn_tto_t S, ttn_tt_t x0, ttn_tt_t x, int64_t n_stages, const int64_t* sweep_schedule,
                         const int64_t* rmax_schedule, int it_solver, int64_t itslv_thresh, int64_t hist_len, double* E) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rb = single_op(A, "ttn_als_gen_eigsolve")) return rb;
    if (int rb = single_op(S, "ttn_als_gen_eigsolve")) return rb;
    return als_eig_impl(1, A, S, x0, x, n_stages, sweep_schedule, rmax_schedule, nullptr, 0, it_solver, 1, TTN_LOBPCG_TOL, itslv_thresh,
                        hist_len, E);
}

// increase_ranks(x, max_bond; rks, noise) (src/tt_tools.jl:443-489; include/ttn_step.h): the stage transition of the one-site eigensolver
// as a call of its own — k_increase_ranks unchanged, its scratch (Tm, Qb, Rb, Vb, Wb, Tst) sized as als_eig_impl sizes it for the new ranks.
int ttn_tt_increase_ranks(ttn_tt_t x, const int64_t* new_rks, double noise, uint64_t seed, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !y || !new_rks) return fail(TTN_ERR_ARG, "null pointer");
    F64_ONLY("ttn_tt_increase_ranks", {x, y});
    if (!same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (x == y) return fail(TTN_ERR_ARG, "ttn_tt_increase_ranks: output must not alias the input");
    if (!(noise >= 0.0 || noise < 0.0) || std::isinf(noise)) return fail(TTN_ERR_ARG, "ttn_tt_increase_ranks: noise is not finite");
    const int d = x->d, batch = x->batch;
    if (new_rks[0] != 1 || new_rks[d] != 1) return fail(TTN_ERR_ARG, "ttn_tt_increase_ranks: the end ranks must be 1");
    int rc = ttn_tt_max_ranks(x, nullptr);                              // the current ranks, not their host-side bound (synchronises)
    if (rc) return rc;
    for (int m = 0; m <= d; ++m) {
        if (new_rks[m] < x->bound[m]) return fail(TTN_ERR_ARG, "ttn_tt_increase_ranks: a new rank is below a current rank");
        if (new_rks[m] > y->cap[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_increase_ranks: a new rank is above the destination's capacity");
    }
    long long mmax = 1, cmax = 1, Nmax = 1;
    for (int i = 0; i < d; ++i) {
        const long long n = x->dims[i], a = new_rks[i], c = new_rks[i + 1];
        Nmax = std::max(Nmax, n * a * c);
        mmax = std::max(mmax, std::max(n * a, n * c));
        cmax = std::max(cmax, std::max(a, c));
    }
    if (noise != 0.0 && (cmax > 1024 || Nmax > 65536))
        return fail(TTN_ERR_UNSUPPORTED, "ttn_tt_increase_ranks: with noise, ranks above 1024 or cores above 65 536 entries are not supported");
    IncArgs Ia;
    memset(&Ia, 0, sizeof(Ia));
    long long cur = 0;
    Ia.offTm = cur; cur += mmax * cmax;
    Ia.offQb = cur; cur += mmax * cmax;
    Ia.offRb = cur; cur += cmax * cmax;
    Ia.offVb = cur; cur += QR_NB * mmax;
    Ia.offWb = cur; cur += QR_NB * mmax;
    Ia.offTst = cur; cur += ((cmax + QR_NB - 1) / QR_NB) * QR_NB * QR_NB + 64;
    const long long per_train = noise != 0.0 ? cur : 1;                 // (zero padding alone touches no scratch)
    if ((rc = scratch_take(sizeof(double) * (size_t)per_train * batch)) || (rc = g_als_tab.ensure(sizeof(long long) * (d + 1)))) return rc;
    std::vector<long long> rn(new_rks, new_rks + d + 1);
    HIPCHK(hipMemcpyAsync(g_als_tab.p, rn.data(), sizeof(long long) * (d + 1), hipMemcpyHostToDevice, g_stream));
    Ia.x = x->dev(); Ia.y = y->dev(); Ia.rn = g_als_tab.as<const long long>();
    Ia.noise = noise; Ia.seed = seed;
    Ia.scratch = g_scratch.as<double>(); Ia.scratch_stride = per_train;
    hipLaunchKernelGGL(k_increase_ranks, dim3(batch), dim3(TTN_WG), COMPRESS_LDS_BYTES, g_stream, Ia);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));                             // rn is a local
    y->bound.assign(new_rks, new_rks + d + 1);
    std::fill(y->ot.begin(), y->ot.end(), 0);
    return TTN_OK;
}

// ---- TT operator algebra (csrc/ttn_opalg_kernels.h) ----------------------------------------------------------------------------
// Every operation allocates its result with tto_alloc (an operator handle is immutable).
// *(A::TToperator, B::TToperator)   src/tt_operations.jl:162-172
int ttn_tto_mul(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_mul", {}, {A, B});
    if (!A || !B || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_mul")) return rb;
    if (int rb = single_op(B, "ttn_tto_mul")) return rb;
    if (!same_dims(A->dims, B->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    const int d = A->d;
    std::vector<int64_t> rks(d + 1);
    for (int m = 0; m <= d; ++m) rks[m] = A->rks[m] * B->rks[m];
    OwnedTTO Y;
    int rc = tto_alloc("ttn_tto_mul", 1, d, A->dims.data(), rks.data(), nullptr, nullptr, Y);
    if (rc) return rc;
    // LDS: the largest binary-site A core that fits; grid: rows x column groups on binary sites, fibres elsewhere
    long long lds_a = 0, items = 1;
    for (int k = 0; k < d; ++k) {
        const long long P = rks[k], Q = rks[k + 1];
        if (A->dims[k] == 2) {
            const long long asz = 4LL * A->rks[k] * A->rks[k + 1];
            if (asz <= TTN_TTOMUL_LDS_DOUBLES) lds_a = std::max(lds_a, asz);
            items = std::max(items, P * ((Q + TTN_TTOMUL_K - 1) / TTN_TTOMUL_K));
        } else items = std::max(items, P * Q);
    }
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    hipLaunchKernelGGL(k_tto_mul, stream_grid(items, d, 1), dim3(TTN_STREAM_TB), sizeof(double) * (size_t)lds_a, g_stream, A->dev(), B->dev(), Y.h->d_data,
                       (const long long*)Y.h->d_off, (int)lds_a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));       // ttn_last_launch_ms: the kernel alone, without this call's allocation
    g_have_launch_ms = true;
    *out = Y.release();
    return TTN_OK;
}

// A ⨝ B   src/tt_operations.jl:198-216
int ttn_tto_inner(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_inner", {}, {A, B});
    if (!A || !B || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_inner")) return rb;
    if (int rb = single_op(B, "ttn_tto_inner")) return rb;
    if (A->d != B->d) return fail(TTN_ERR_DIMS, "Inner core product requires operators with the same number of cores");
    const int d = A->d;
    std::vector<int64_t> rks(d + 1), dims(d);
    for (int m = 0; m <= d; ++m) rks[m] = A->rks[m] * B->rks[m];
    long long items = 1;
    for (int k = 0; k < d; ++k) {
        dims[k] = A->dims[k] * B->dims[k];
        if (dims[k] > 46340) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_inner: physical dimension above 46340");
        items = std::max<long long>(items, std::min<long long>((long long)dims[k] * dims[k] * std::min<long long>(rks[k] * rks[k + 1], 1LL << 31), 1LL << 40));
    }
    OwnedTTO Y;
    int rc = tto_alloc("ttn_tto_inner", 1, d, dims.data(), rks.data(), nullptr, nullptr, Y);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tto_inner, stream_grid(items, d, 1), dim3(TTN_STREAM_TB), 0, g_stream, A->dev(), B->dev(), Y.h->d_data, (const long long*)Y.h->d_off);
    HIPCHK(hipGetLastError());
    *out = Y.release();
    return TTN_OK;
}

// +(x::TToperator, y::TToperator)   src/tt_operations.jl:71-95: k_add on the operators seen as vectors
int ttn_tto_add(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_add", {}, {A, B});
    if (!A || !B || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_add")) return rb;
    if (int rb = single_op(B, "ttn_tto_add")) return rb;
    if (!same_dims(A->dims, B->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    const int d = A->d;
    if (d < 2) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_add: the reference's + is only defined for d >= 2");
    std::vector<int64_t> rks(d + 1);
    for (int m = 0; m <= d; ++m) rks[m] = (m == 0 || m == d) ? 1 : A->rks[m] + B->rks[m];
    OwnedTTO Z;
    int rc = tto_alloc("ttn_tto_add", 1, d, A->dims.data(), rks.data(), nullptr, nullptr, Z);
    if (rc) return rc;
    launch_add(A->vdev(), B->vdev(), Z.h->vdev(), rks, false, 1);     // k_add's n = 2 mapping is for vector dims 2: the n^2 of an operator is never 2
    HIPCHK(hipGetLastError());
    *out = Z.release();
    return TTN_OK;
}

// *(a::Number, A::TToperator)   src/tt_operations.jl:271-281: k_scale on the operator seen as a vector
int ttn_tto_scale(double a, ttn_tto_t A, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_scale", {}, {A});
    if (!A || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_scale")) return rb;
    const int d = A->d;
    std::vector<int64_t> ot(A->ot);
    if (a == 0.0) std::fill(ot.begin(), ot.end(), 0);       // zeros_tto(dims, rks)
    OwnedTTO Y;
    int rc = tto_alloc("ttn_tto_scale", 1, d, A->dims.data(), A->rks.data(), ot.data(), nullptr, Y);
    if (rc) return rc;
    int which = 0;
    const int* which_b = nullptr;                           // one train: stays null
    if ((rc = scaled_core(A->ot.data(), d, 1, which, which_b))) return rc;
    std::vector<int64_t> dims2(d);
    for (int k = 0; k < d; ++k) dims2[k] = A->dims[k] * A->dims[k];
    launch_scale(1, d, 1, dims2.data(), A->rks.data(), A->vdev(), Y.h->vdev(), a, 0.0, nullptr, which, which_b, a == 0.0);
    HIPCHK(hipGetLastError());
    *out = Y.release();
    return TTN_OK;
}

// kron(A, B) (src/tt_operations.jl:427-433) and concatenate(A, B) (src/tt_tools.jl:723-735): B's cores behind A's, two device copies
int ttn_tto_kron(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_kron", {}, {A, B});
    if (!A || !B || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_kron")) return rb;
    if (int rb = single_op(B, "ttn_tto_kron")) return rb;
    if (A->rks[A->d] != B->rks[0]) return fail(TTN_ERR_DIMS, "The final rank of the first TToperator must equal the initial rank of the second TToperator.");
    const int d = A->d + B->d;
    std::vector<int64_t> dims(A->dims), rks(A->rks.begin(), A->rks.end() - 1), ot(A->ot);
    dims.insert(dims.end(), B->dims.begin(), B->dims.end());
    rks.insert(rks.end(), B->rks.begin(), B->rks.end());
    ot.insert(ot.end(), B->ot.begin(), B->ot.end());
    OwnedTTO Y;
    int rc = tto_alloc("ttn_tto_kron", 1, d, dims.data(), rks.data(), ot.data(), nullptr, Y);
    if (rc) return rc;
    // the slot offsets of a handle are running sums of its 16-byte rounded core sizes: the arena of A, then the arena of B
    if (A->off[A->d]) HIPCHK(hipMemcpyAsync(Y.h->d_data, A->d_data, sizeof(double) * (size_t)A->off[A->d], hipMemcpyDeviceToDevice, g_stream));
    if (B->off[B->d]) HIPCHK(hipMemcpyAsync(Y.h->d_data + A->off[A->d], B->d_data, sizeof(double) * (size_t)B->off[B->d], hipMemcpyDeviceToDevice, g_stream));
    *out = Y.release();
    return TTN_OK;
}

// Current ranks of train b of x on the host (synchronises), as the ranks of a new operator
static int train_ranks(ttn_tt_t x, int64_t b, std::vector<int64_t>& rks) {
    rks.resize(x->d + 1);
    return ttn_tt_ranks(x, b, rks.data(), nullptr);
}

// outer_product(x, y)   src/tt_operations.jl:297-304 (real)
int ttn_tt_outer(ttn_tt_t x, ttn_tt_t y, int64_t b, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_outer", {x, y});
    if (!x || !y || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (b < 0 || b >= x->batch || b >= y->batch) return fail(TTN_ERR_ARG, "ttn_tt_outer: train index outside the batch");
    if (!same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    const int d = x->d;
    std::vector<int64_t> xr, yr, rks(d + 1);
    int rc;
    if ((rc = train_ranks(x, b, xr)) || (rc = train_ranks(y, b, yr))) return rc;
    long long items = 1;
    for (int m = 0; m <= d; ++m) rks[m] = xr[m] * yr[m];
    for (int k = 0; k < d; ++k) items = std::max<long long>(items, std::min<long long>((long long)x->dims[k] * x->dims[k] * std::min<long long>(rks[k] * rks[k + 1], 1LL << 31), 1LL << 40));
    OwnedTTO Y;
    if ((rc = tto_alloc("ttn_tt_outer", 1, d, x->dims.data(), rks.data(), nullptr, nullptr, Y))) return rc;
    hipLaunchKernelGGL(k_tt_outer, stream_grid(items, d, 1), dim3(TTN_STREAM_TB), 0, g_stream, x->dev(), y->dev(), (int)b, Y.h->d_data, (const long long*)Y.h->d_off);
    HIPCHK(hipGetLastError());
    *out = Y.release();
    return TTN_OK;
}

// ttv_to_diag_tto(x)   src/tt_operations.jl:310-338
int ttn_tt_diag_tto(ttn_tt_t x, int64_t b, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_diag_tto", {x});
    if (!x || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (b < 0 || b >= x->batch) return fail(TTN_ERR_ARG, "ttn_tt_diag_tto: train index outside the batch");
    const int d = x->d;
    std::vector<int64_t> rks;
    int rc;
    if ((rc = train_ranks(x, b, rks))) return rc;
    long long items = 1;
    for (int k = 0; k < d; ++k) items = std::max<long long>(items, std::min<long long>((long long)x->dims[k] * x->dims[k] * std::min<long long>(rks[k] * rks[k + 1], 1LL << 31), 1LL << 40));
    OwnedTTO Y;
    if ((rc = tto_alloc("ttn_tt_diag_tto", 1, d, x->dims.data(), rks.data(), nullptr, nullptr, Y))) return rc;
    hipLaunchKernelGGL(k_tt_diag, stream_grid(items, d, 1), dim3(TTN_STREAM_TB), 0, g_stream, x->dev(), (int)b, Y.h->d_data, (const long long*)Y.h->d_off);
    HIPCHK(hipGetLastError());
    *out = Y.release();
    return TTN_OK;
}

// kron(a::TTvector, b::TTvector)   src/tt_operations.jl:440-448, train by train: z_b = x_b (x) y_b.  Strided device copies of the slots
// (a slot holds its core compactly at its start: copying the host-side bound of the ranks covers it) and of the rank tables.
int ttn_tt_kron(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tt_kron", {x, y, z});
    if (!x || !y || !z) return fail(TTN_ERR_ARG, "null handle");
    if (z == x || z == y) return fail(TTN_ERR_ARG, "ttn_tt_kron: output must not alias an input");
    const int dx = x->d, dy = y->d, d = dx + dy;
    std::vector<int64_t> dims(x->dims);
    dims.insert(dims.end(), y->dims.begin(), y->dims.end());
    if (z->d != d || !same_dims(z->dims, dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch || x->batch != z->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    if (x->bound[dx] != 1 || y->bound[0] != 1) return fail(TTN_ERR_DIMS, "ttn_tt_kron: the ranks at the joint must be 1");
    std::vector<int64_t> zb(x->bound.begin(), x->bound.end() - 1);
    zb.insert(zb.end(), y->bound.begin(), y->bound.end());
    for (int m = 0; m <= d; ++m) if (z->cap[m] < zb[m]) return fail(TTN_ERR_CAPACITY, "ttn_tt_kron: destination capacity too small");
    const size_t B = (size_t)x->batch;
    for (int k = 0; k < d; ++k) {
        ttn_tt_t s = k < dx ? x : y;
        const int ks = k < dx ? k : k - dx;
        const size_t w = sizeof(double) * (size_t)s->dims[ks] * s->bound[ks] * s->bound[ks + 1];
        HIPCHK(hipMemcpy2DAsync(z->d_data + z->off[k], sizeof(double) * (size_t)z->stride, s->d_data + s->off[ks], sizeof(double) * (size_t)s->stride, w, B,
                                hipMemcpyDeviceToDevice, g_stream));
    }
    HIPCHK(hipMemcpy2DAsync(z->d_rks, sizeof(long long) * (d + 1), x->d_rks, sizeof(long long) * (dx + 1), sizeof(long long) * dx, B, hipMemcpyDeviceToDevice, g_stream));
    HIPCHK(hipMemcpy2DAsync(z->d_rks + dx, sizeof(long long) * (d + 1), y->d_rks, sizeof(long long) * (dy + 1), sizeof(long long) * (dy + 1), B, hipMemcpyDeviceToDevice, g_stream));
    z->bound = zb;
    for (size_t b = 0; b < B; ++b)
        for (int k = 0; k < d; ++k) z->ot[b * d + k] = k < dx ? x->ot[b * dx + k] : y->ot[b * dy + (k - dx)];
    return TTN_OK;
}

// tto_to_ttv(A) (src/tt_tools.jl:296-304) into every train of y: one device copy per core into train 0, then ttn_tt_replicate
int ttn_tto_to_tt(ttn_tto_t A, ttn_tt_t y) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_to_tt", {y}, {A});
    if (!A || !y) return fail(TTN_ERR_ARG, "null handle");
    if (int rb = single_op(A, "ttn_tto_to_tt")) return rb;
    const int d = A->d;
    if (y->d != d) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    for (int k = 0; k < d; ++k) if (y->dims[k] != A->dims[k] * A->dims[k]) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    for (int m = 0; m <= d; ++m) if (y->cap[m] < A->rks[m]) return fail(TTN_ERR_CAPACITY, "ttn_tto_to_tt: destination capacity too small");
    for (int k = 0; k < d; ++k) {
        const size_t sz = (size_t)y->dims[k] * A->rks[k] * A->rks[k + 1];
        HIPCHK(hipMemcpyAsync(y->d_data + y->off[k], A->d_data + A->off[k], sizeof(double) * sz, hipMemcpyDeviceToDevice, g_stream));
    }
    HIPCHK(hipMemcpyAsync(y->d_rks, A->d_rks, sizeof(long long) * (d + 1), hipMemcpyDeviceToDevice, g_stream));
    for (int k = 0; k < d; ++k) y->ot[k] = A->ot[k];
    y->bound = A->rks;
    return ttn_tt_replicate(y, 0);
}

// ttv_to_tto(x_b) (src/tt_tools.jl:323-333) with the train's current ranks (synchronises to read them)
int ttn_tto_from_tt(ttn_tt_t x, int64_t b, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_from_tt", {x});
    if (!x || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (b < 0 || b >= x->batch) return fail(TTN_ERR_ARG, "ttn_tto_from_tt: train index outside the batch");
    const int d = x->d;
    std::vector<int64_t> dims(d), rks;
    for (int k = 0; k < d; ++k) {
        dims[k] = (int64_t)std::llround(std::sqrt((double)x->dims[k]));
        if (dims[k] * dims[k] != x->dims[k]) return fail(TTN_ERR_DIMS, "DimensionMismatch: the dimensions of the train are not perfect squares");
    }
    int rc;
    if ((rc = train_ranks(x, b, rks))) return rc;
    OwnedTTO Y;
    if ((rc = tto_alloc("ttn_tto_from_tt", 1, d, dims.data(), rks.data(), x->ot.data() + (size_t)b * d, nullptr, Y))) return rc;
    for (int k = 0; k < d; ++k) {
        const size_t sz = (size_t)x->dims[k] * rks[k] * rks[k + 1];
        HIPCHK(hipMemcpyAsync(Y.h->d_data + Y.h->off[k], x->d_data + (size_t)b * x->stride + x->off[k], sizeof(double) * sz, hipMemcpyDeviceToDevice, g_stream));
    }
    *out = Y.release();
    return TTN_OK;
}

// tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps) as an operator again: to_tt -> ttn_compress -> from_tt on the device.  The
// working train is read and cleared of its status here (a failure is this call's return value), so its release folds nothing into
// the library-level word of ttn_status_all.
int ttn_tto_compress(ttn_tto_t A, int64_t max_bond, double truncerr, int64_t sweeps, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_compress", {}, {A});
    if (!A || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_tto_compress")) return rb;
    if (sweeps < 1) return fail(TTN_ERR_SWEEPS, "sweeps must be >= 1");
    if (max_bond < 1) return fail(TTN_ERR_ARG, "max_bond must be >= 1");
    const int d = A->d;
    std::vector<int64_t> dims2(d), need, fin;
    for (int k = 0; k < d; ++k) dims2[k] = A->dims[k] * A->dims[k];
    long long pm, qm;
    rank_bounds(d, dims2.data(), A->rks.data(), max_bond, sweeps, 0, need, fin, pm, qm);
    OwnedTT t;
    int rc;
    if ((rc = ttn_tt_create(d, dims2.data(), need.data(), 1, &t.h))) return rc;
    if ((rc = ttn_tto_to_tt(A, t.h))) return rc;
    if ((rc = ttn_compress(t.h, max_bond, truncerr, sweeps))) return rc;
    if ((rc = ttn_compress_status(t.h, nullptr))) return rc;
    return ttn_tto_from_tt(t.h, 0, out);
}

// ---- operator batches (include/ttn_opbatch.h, csrc/ttn_opbatch_kernels.h) -------------------------------------------------------------
int ttn_tto_create_batch(int64_t d, const int64_t* dims, const int64_t* rks, int64_t batch, const double* const* cores, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!dims || !rks || !cores || !out || d < 1 || batch < 1) return fail(TTN_ERR_ARG, "ttn_tto_create_batch: bad argument");
    for (int64_t k = 0; k < d; ++k) if (dims[k] < 1) return fail(TTN_ERR_ARG, "ttn_tto_create_batch: dims must be >= 1");
    for (int64_t m = 0; m <= d; ++m) if (rks[m] < 1) return fail(TTN_ERR_ARG, "ttn_tto_create_batch: ranks must be >= 1");
    for (int64_t e = 0; e < batch * d; ++e) if (!cores[e]) return fail(TTN_ERR_ARG, "ttn_tto_create_batch: null core");
    OwnedTTO A;
    const int rc = tto_alloc(nullptr, 1, d, dims, rks, nullptr, cores, A, batch);
    if (rc) return rc;
    *out = A.release();
    return TTN_OK;
}

int ttn_tto_from_tt_batch(ttn_tt_t v, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    F64_ONLY("ttn_tto_from_tt_batch", {v});
    if (!v || !out) return fail(TTN_ERR_ARG, "null pointer");
    const int d = v->d, batch = v->batch;
    std::vector<int64_t> dims(d), rks(d + 1);
    for (int k = 0; k < d; ++k) {
        dims[k] = (int64_t)std::llround(std::sqrt((double)v->dims[k]));
        if (dims[k] * dims[k] != v->dims[k]) return fail(TTN_ERR_DIMS, "DimensionMismatch: the dimensions of the train are not perfect squares");
    }
    // the one rank read: every train must hold the ranks of train 0 (they become the host-known ranks of the batch)
    std::vector<long long> r64((size_t)batch * (d + 1));
    HIPCHK(hipMemcpyAsync(r64.data(), v->d_rks, sizeof(long long) * r64.size(), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int b = 1; b < batch; ++b)
        for (int m = 0; m <= d; ++m)
            if (r64[(size_t)b * (d + 1) + m] != r64[m])
                return fail(TTN_ERR_DIMS, ("ttn_tto_from_tt_batch: the ranks of train " + std::to_string(b) + " differ from those of train 0 at bond " + std::to_string(m)
                                           + " (" + std::to_string(r64[(size_t)b * (d + 1) + m]) + " against " + std::to_string(r64[m]) + "): one operator batch holds equal ranks").c_str());
    long long maxsz = 1;
    for (int m = 0; m <= d; ++m) {
        rks[m] = r64[m];
        if (rks[m] < 1 || rks[m] > v->cap[m]) return fail(TTN_ERR_CAPACITY, "ttn_tto_from_tt_batch: a rank of the trains is outside the capacity of their handle");
    }
    for (int k = 0; k < d; ++k) maxsz = std::max<long long>(maxsz, (long long)v->dims[k] * rks[k] * rks[k + 1]);
    bool same_ot = true;
    for (int b = 1; b < batch; ++b) for (int k = 0; k < d; ++k) same_ot = same_ot && v->ot[(size_t)b * d + k] == v->ot[k];
    OwnedTTO Y;
    int rc;
    if ((rc = tto_alloc("ttn_tto_from_tt_batch", 1, d, dims.data(), rks.data(), same_ot ? v->ot.data() : nullptr, nullptr, Y, batch))) return rc;
    if (!g_poison)                                                     // the rounding gaps of odd cores (poison mode: tto_alloc's pattern stays in them)
        HIPCHK(hipMemsetAsync(Y.h->d_data, 0, sizeof(double) * (size_t)std::max<long long>(Y.h->stride, 1) * batch, g_stream));
    TTODev dst = Y.h->dev();
    dst.stride = Y.h->stride;
    hipLaunchKernelGGL(k_tto_pack, stream_grid((maxsz + 1) / 2, d, batch), dim3(TTN_STREAM_TB), 0, g_stream, v->dev(), dst, Y.h->d_data);
    HIPCHK(hipGetLastError());
    *out = Y.release();
    return TTN_OK;
}

int ttn_tto_batch(ttn_tto_t A, int64_t* batch) {
    if (!A || !batch) return fail(TTN_ERR_ARG, "null pointer");
    *batch = A->batch;
    return TTN_OK;
}

int ttn_tto_select(ttn_tto_t A, int64_t b, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (b < 0 || b >= A->batch) return fail(TTN_ERR_ARG, "ttn_tto_select: operator index outside the batch");
    OwnedTTO Y;
    int rc;
    if ((rc = tto_alloc("ttn_tto_select", A->el, A->d, A->dims.data(), A->rks.data(), A->ot.data(), nullptr, Y))) return rc;
    if (A->stride) HIPCHK(hipMemcpyAsync(Y.h->d_data, A->d_data + (size_t)b * A->stride, sizeof(double) * (size_t)A->stride, hipMemcpyDeviceToDevice, g_stream));
    *out = Y.release();
    return TTN_OK;
}

int ttn_tto_download_b(ttn_tto_t A, int64_t b, double* const* cores) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!A || !cores) return fail(TTN_ERR_ARG, "null pointer");
    if (b < 0 || b >= A->batch) return fail(TTN_ERR_ARG, "ttn_tto_download_b: operator index outside the batch");
    for (int k = 0; k < A->d; ++k) {
        if (!cores[k]) return fail(TTN_ERR_ARG, "ttn_tto_download_b: null core");
        const size_t sz = (size_t)A->el * A->dims[k] * A->dims[k] * A->rks[k] * A->rks[k + 1];
        HIPCHK(hipMemcpyAsync(cores[k], A->d_data + (size_t)b * A->stride + A->off[k], sizeof(double) * sz, hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

// tto_decomp(tensor; index) from a dense array on the device (include/ttn_dense.h): k_dense_gather permutes the array into the layout
// (n_1^2, ..., n_d^2) of tto_decomp's reshape(permutedims(...)) in a temporary allocation, ttv_decomp runs on a working train that is
// read and cleared of its status here (a failure is this call's return value, as in ttn_tto_compress), then from_tt.
int ttn_tto_decomp_dev(int64_t d64, const int64_t* dims, const double* d_tensor, const int64_t* xstrides, const int64_t* ystrides, int64_t index,
                       double tol, int64_t rank_cap, ttn_tto_t* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    const char* who = "ttn_tto_decomp_dev";
    if (!dims || !d_tensor || !out) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: null argument");
    if (d64 < 1 || d64 > TTN_MAX_D) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: the number of sites must be in 1:64");
    const int d = (int)d64;
    if ((xstrides == nullptr) != (ystrides == nullptr)) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: xstrides and ystrides must both be given or both be null");
    if (index < 1 || index > d) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: index must be in 1:d");
    if (!(tol >= 0.0)) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: tol must be >= 0");
    if (rank_cap < 1) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: rank_cap must be >= 1");
    std::vector<int64_t> dims2(d);
    long long total = 1;
    for (int k = 0; k < d; ++k) {
        if (dims[k] < 1) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: dims must be >= 1");
        if (dims[k] > TTN_DENSE_TILE) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_decomp_dev: a physical dimension above 4096");
        dims2[k] = dims[k] * dims[k];
        total *= dims2[k];
        if (total > (1LL << 27)) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_decomp_dev: more than 2^27 entries");
    }
    // the digits x_1, y_1, x_2, y_2, ... with their strides in the caller's array and in the array the decomposition reads
    std::vector<long long> xs, ys;
    operator_strides(d, dims, xstrides, ystrides, xs, ys);
    std::vector<int> dn(2 * d);
    std::vector<long long> din(2 * d), dout(2 * d);
    { long long s = 1; for (int k = 0; k < d; ++k) { dn[2 * k] = dn[2 * k + 1] = (int)dims[k]; din[2 * k] = xs[k]; din[2 * k + 1] = ys[k];
                                                      dout[2 * k] = s; dout[2 * k + 1] = s * dims[k]; s *= dims2[k]; } }
    std::vector<int> iord, oord;
    if (!mixed_radix_order(dn, din, iord)) return fail(TTN_ERR_ARG, "ttn_tto_decomp_dev: the strides are not a mixed-radix system (smallest 1, each next = previous * its n)");
    mixed_radix_order(dn, dout, oord);
    // capacity of the working train, and the limits of the decomposition under it
    std::vector<int64_t> cap(d + 1, 1), bnd;
    { long long p = 1; for (int k = 1; k < d; ++k) { p *= dims2[k - 1]; cap[k] = std::min<long long>(std::min<long long>(p, total / p), rank_cap); } }
    long long tot2, pmax, qmax;
    int rc;
    if ((rc = ttv_decomp_plan(who, "lower rank_cap", d, dims2.data(), cap.data(), index, bnd, tot2, pmax, qmax))) return rc;
    if (iord.size() > TTN_GATHER_DIGITS) return fail(TTN_ERR_UNSUPPORTED, "ttn_tto_decomp_dev: too many digits");     // (2^27 entries leave at most 27)
    // ---- the tile of the gather ----
    std::vector<char> in_tile(2 * d, 0);
    std::vector<int> SI, SO;
    long long TI = 1, TO = 1;
    size_t ip = 0;
    while (ip < iord.size() && (TI < 64 || SI.empty()) && TI * dn[iord[ip]] <= TTN_DENSE_TILE) { TI *= dn[iord[ip]]; in_tile[iord[ip]] = 1; SI.push_back(iord[ip]); ++ip; }
    for (int j : oord) {
        if (in_tile[j]) continue;
        if (TI * TO * dn[j] > TTN_DENSE_TILE) break;
        TO *= dn[j]; in_tile[j] = 2; SO.push_back(j);
    }
    while (ip < iord.size() && !in_tile[iord[ip]] && TI * TO * dn[iord[ip]] <= TTN_DENSE_TILE) { TI *= dn[iord[ip]]; in_tile[iord[ip]] = 1; SI.push_back(iord[ip]); ++ip; }
    // eh enumerates SO in output order (as collected): the digits that vary inside a half wave of the store phase then get the small
    // weights, and the pad below can spread them over the banks
    const int nt = (int)(TI * TO);
    // LDS position strides for ld = TI + pad: an SI digit keeps its input stride, an SO digit gets ld times its weight in eh
    auto lds_strides = [&](long long ld, std::vector<long long>& ls) {
        ls.assign(2 * d, 0);
        for (int j : SI) ls[j] = din[j];
        long long w = 1;
        for (int j : SO) { ls[j] = ld * w; w *= dn[j]; }
    };
    // the tile's digits in output order: the leading ones that follow each other without a gap span runs of RO contiguous outputs
    std::vector<int> lo, hi;
    long long RO = 1;
    { bool run = true; for (int j : oord) { if (!in_tile[j]) { run = false; continue; } if (run) { lo.push_back(j); RO *= dn[j]; } else hi.push_back(j); } }
    const long long FH = nt / RO;
    // the pad: the fewest bank conflicts of the store phase's LDS reads (8-byte reads: 32 banks of doubles, lanes in halves of 32), over
    // the first 256 elements; ties go to the smaller pad
    long long ld = TI;
    {
        long long best = -1;
        std::vector<long long> ls;
        for (long long pad = 0; pad <= 32 && TO * (TI + pad) <= TTN_GATHER_LDS; ++pad) {
            lds_strides(TI + pad, ls);
            long long cost = 0;
            for (int f0 = 0; f0 < std::min(nt, 256); f0 += 32) {
                int cnt[32] = {0};
                for (int f = f0; f < std::min(nt, f0 + 32); ++f) {
                    long long rem = f, pos = 0;
                    for (int j : lo) { pos += (rem % dn[j]) * ls[j]; rem /= dn[j]; }
                    for (int j : hi) { pos += (rem % dn[j]) * ls[j]; rem /= dn[j]; }
                    ++cnt[pos & 31];
                }
                int worst = 0;
                for (int c : cnt) worst = std::max(worst, c);
                cost += worst;
            }
            if (best < 0 || cost < best) { best = cost; ld = TI + pad; }
            if (TO == 1) break;                                 // one row: the pad changes nothing
        }
        // diagnostic knob (tools/diag_dense_operator.py measures what the search is worth): TTN_GATHER_PAD = a fixed pad instead
        if (const char* e = getenv("TTN_GATHER_PAD")) { const long long pad = atoll(e); if (pad >= 0 && pad <= 32 && TO * (TI + pad) <= TTN_GATHER_LDS) ld = TI + pad; }
    }
    std::vector<long long> ls;
    lds_strides(ld, ls);
    // ---- temporary device memory: [permuted array | inHi | outHi | posLo | posHi (+ the off / idx halves k_dense_tables also fills)] ----
    struct Temp { void* p = nullptr; ~Temp() { if (p) { hipStreamSynchronize(g_stream); hipFree(p); } } } tmp;
    auto pad2 = [](long long v) { return (v + 1) & ~1LL; };
    const long long o_inHi = pad2(total), o_inIdx = o_inHi + TO, o_loOff = o_inIdx + pad2((TO + 1) / 2), o_loIdx = o_loOff + RO,
                    o_hiOff = o_loIdx + pad2((RO + 1) / 2), o_hiIdx = o_hiOff + FH, o_end = o_hiIdx + pad2((FH + 1) / 2);
    if (hipMalloc(&tmp.p, sizeof(double) * (size_t)o_end) != hipSuccess) {
        (void)hipGetLastError();
        tmp.p = nullptr;
        return fail(TTN_ERR_CAPACITY, "ttn_tto_decomp_dev: the permuted array does not fit in device memory");
    }
    double* base = static_cast<double*>(tmp.p);
    auto fill_table = [&](const std::vector<int>& dg, const std::vector<long long>& stride, long long count, long long o_off, long long o_idx) {
        DenseTabArgs T;
        memset(&T, 0, sizeof(T));
        for (int j : dg) { T.n[T.ns] = dn[j]; T.stride[T.ns] = stride[j]; T.rstride[T.ns] = ls[j]; ++T.ns; }
        T.count = count; T.off = reinterpret_cast<long long*>(base + o_off); T.idx = reinterpret_cast<int*>(base + o_idx);
        const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((count + TTN_DENSE_TB - 1) / TTN_DENSE_TB, 1024));
        hipLaunchKernelGGL(k_dense_tables, dim3(blocks), dim3(TTN_DENSE_TB), 0, g_stream, T);
    };
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    fill_table(SO, din, TO, o_inHi, o_inIdx);
    fill_table(lo, dout, RO, o_loOff, o_loIdx);
    fill_table(hi, dout, FH, o_hiOff, o_hiIdx);
    GatherArgs G;
    memset(&G, 0, sizeof(G));
    G.in = d_tensor; G.out = base;
    G.TI = (int)TI; G.TO = (int)TO; G.ld = (int)ld; G.RO = (int)RO; G.nt = nt;
    g_gather_plan[0] = TI; g_gather_plan[1] = TO; g_gather_plan[2] = ld; g_gather_plan[3] = RO;
    G.inHi = reinterpret_cast<const long long*>(base + o_inHi);
    G.posLo = reinterpret_cast<const int*>(base + o_loIdx);
    G.outHi = reinterpret_cast<const long long*>(base + o_hiOff);
    G.posHi = reinterpret_cast<const int*>(base + o_hiIdx);
    for (int j : iord) {
        if (in_tile[j]) continue;
        G.on[G.nouter] = dn[j]; G.oin[G.nouter] = din[j]; G.oout[G.nouter] = dout[j]; ++G.nouter;
    }
    hipLaunchKernelGGL(k_dense_gather, dim3((unsigned)(total / nt)), dim3(TTN_DENSE_TB), 0, g_stream, G);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));       // ttn_last_launch_ms: the gather (its tables and the kernel) without the decomposition
    g_have_launch_ms = true;
    // ---- the decomposition on a working train, then the operator ----
    OwnedTT t;
    if ((rc = ttn_tt_create(d, dims2.data(), cap.data(), 1, &t.h))) return rc;
    if ((rc = ttn_ttv_decomp_dev(t.h, base, index, tol))) return rc;
    unsigned seen = 0;
    if ((rc = take_status(t.h, seen))) return rc;
    if ((rc = status_error(seen, who))) return rc;
    return ttn_tto_from_tt(t.h, 0, out);
}

// ---- version, errors, ttn_init / ttn_finalize, sync, timers and event slots ------------------------------------------------------
// Last: ttn_finalize is the one teardown and names the state of every module, in this file and in the host headers.
static hipEvent_t g_ev0 = nullptr, g_ev1 = nullptr;                 // ttn_timer_begin / ttn_timer_end
static std::vector<hipEvent_t> g_slots;   // ttn_event_record slots
const char* ttn_version(void) { return "ttn-mi355x 0.1.0 (gfx950, fp64)"; }
const char* ttn_last_error_string(void) { return g_err.c_str(); }

int ttn_device_count(int* n) {
    if (!n) return fail(TTN_ERR_ARG, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return hipfail(e, "hipGetDeviceCount"); }
    *n = c;
    return TTN_OK;
}

int ttn_init(int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (g_init && device == g_device) return TTN_OK;
    if (g_init) return fail(TTN_ERR_ARG, "ttn_init: already bound to another device (call ttn_finalize first)");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&g_ev0, &g_ev1, &g_launch_ev0, &g_launch_ev1}) HIPCHK(hipEventCreate(e));
    for (const auto& a : lds_limits) HIPCHK(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds));
    { const int rc512 = ttn_wg512_init(); if (rc512) return hipfail((hipError_t)rc512, "ttn_wg512_init"); }
    if (ttn_wg512_compress_args_bytes() != sizeof(CompressArgs)) return fail(TTN_ERR_ARG, "ttn_init: the two kernel builds disagree on CompressArgs");
    { int rc = g_next_train.ensure(sizeof(int)); if (rc) return rc; }
    { int rc = g_pending_status.ensure(sizeof(unsigned)); if (rc) return rc; }
    HIPCHK(hipMemset(g_pending_status.p, 0, sizeof(unsigned)));
    g_device = device;
    g_init = true;
    return TTN_OK;
}

int ttn_finalize(void) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!g_init) return TTN_OK;
    hipStreamSynchronize(g_stream);
    for (DevBuf* b = DevBuf::head; b; b = b->next) b->release();
    for (hipEvent_t e : {g_ev0, g_ev1, g_launch_ev0, g_launch_ev1}) hipEventDestroy(e);
    g_have_launch_ms = false;
    g_ortho_state_batch = 0;
    g_poison = false;                   // a test switch does not outlive the library state it was set on
    for (auto e : g_slots) if (e) hipEventDestroy(e);
    g_slots.clear();
    if (g_xb_tab_ev) { hipEventDestroy(g_xb_tab_ev); g_xb_tab_ev = nullptr; }
    if (g_measure_ev) { hipEventDestroy(g_measure_ev); g_measure_ev = nullptr; }
    if (g_contract_ev) { hipEventDestroy(g_contract_ev); g_contract_ev = nullptr; }
    if (g_zmeasure_ev) { hipEventDestroy(g_zmeasure_ev); g_zmeasure_ev = nullptr; }
    for (hipEvent_t e : g_sample_ev) hipEventDestroy(e);
    g_sample_ev.clear();
    g_sample_chunks = 0;
    hipStreamDestroy(g_stream);
    g_stream = nullptr; g_init = false; g_device = -1;
    return TTN_OK;
}

int ttn_sync(void) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}

int ttn_timer_begin(void) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    HIPCHK(hipEventRecord(g_ev0, g_stream));
    return TTN_OK;
}
int ttn_timer_end(float* ms) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!ms) return fail(TTN_ERR_ARG, "null pointer");
    HIPCHK(hipEventRecord(g_ev1, g_stream));
    HIPCHK(hipEventSynchronize(g_ev1));
    HIPCHK(hipEventElapsedTime(ms, g_ev0, g_ev1));
    return TTN_OK;
}

int ttn_event_record(int64_t slot) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (slot < 0 || slot >= 4096) return fail(TTN_ERR_ARG, "event slot out of range");
    if ((int64_t)g_slots.size() <= slot) g_slots.resize(slot + 1, nullptr);
    if (!g_slots[slot]) HIPCHK(hipEventCreate(&g_slots[slot]));
    HIPCHK(hipEventRecord(g_slots[slot], g_stream));
    return TTN_OK;
}
int ttn_event_elapsed(int64_t a, int64_t b, float* ms) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!ms || a < 0 || b < 0 || a >= (int64_t)g_slots.size() || b >= (int64_t)g_slots.size() || !g_slots[a] || !g_slots[b])
        return fail(TTN_ERR_ARG, "event slot not recorded");
    HIPCHK(hipEventSynchronize(g_slots[b]));
    HIPCHK(hipEventElapsedTime(ms, g_slots[a], g_slots[b]));
    return TTN_OK;
}
}  // extern "C"
