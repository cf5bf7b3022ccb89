// ttn_host_braket.h — host API: <x| A |y> with x conjugated, on ComplexF64 or Float64 operands (include/ttn_braket.h).
#ifndef TTN_HOST_BRAKET_H
#define TTN_HOST_BRAKET_H
#include "ttn_host_core.h"
#include "ttn_host_dot.h"
#include "ttn_braket_kernels.h"

namespace {
DevBuf g_braket_real;      // [batch] doubles: what k_expect writes when all three operands are Float64

// out[b] = (in[b], +0.0): the all-Float64 form of ttn_braket
__global__ void k_braket_widen(const double* in, double* out, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) { out[2 * b] = in[b]; out[2 * b + 1] = 0.0; }
}
template <bool CA, bool CX>
static void braket_dispatch(int rm, dim3 grid, dim3 block, size_t lds, const BraketArgs& P) {
    switch (rm) {
        case 1: hipLaunchKernelGGL((k_zexpect<CA, CX, 1>), grid, block, lds, g_stream, P); break;
        case 2: hipLaunchKernelGGL((k_zexpect<CA, CX, 2>), grid, block, lds, g_stream, P); break;
        default: hipLaunchKernelGGL((k_zexpect<CA, CX, 0>), grid, block, lds, g_stream, P); break;
    }
}
static_assert(BRAKET_QTT_OPR_MAX == 2, "braket_dispatch and the table of ttn_host_lds.h list one kernel per operator rank of the on-chip route");
}  // namespace

extern "C" {
static_assert(BRAKET_QTT_RMAX == TTN_BRAKET_QTT_MAX_RANK && BRAKET_QTT_OPR_MAX == TTN_BRAKET_QTT_MAX_OP_RANK, "ttn_braket.h and ttn_braket_kernels.h disagree");

// Every refusal of the call, under the caller's name `who`, before any allocation or launch; A is one operator (the entry points have
// refused a batch).  The all-Float64 form is k_expect's launch: its workspace counts one double per element, the others two.
static int braket_check(const char* who, ttn_tt_t x, ttn_tto_t A, ttn_tt_t y) {
    if (x->el != y->el) return refuse_mixed(who);
    if (!same_dims(A->dims, x->dims) || !same_dims(x->dims, y->dims)) return fail(TTN_ERR_DIMS, "Incompatible dimensions");
    if (x->batch != y->batch) return fail(TTN_ERR_DIMS, "batch sizes differ");
    const std::string w(who);
    const int d = x->d;
    if (d > BRAKET_MAX_D) return fail(TTN_ERR_UNSUPPORTED, (w + ": chains longer than 480 sites are not supported").c_str());
    if (x->stride >= (1LL << 31) || y->stride >= (1LL << 31) || A->off.back() >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, (w + ": a train or an operator of 2^31 doubles or more").c_str());
    long long rxmax = 1, rymax = 1, Rmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) {
        rxmax = std::max<long long>(rxmax, x->bound[m]); rymax = std::max<long long>(rymax, y->bound[m]); Rmax = std::max<long long>(Rmax, A->rks[m]);
    }
    for (int k = 0; k < d; ++k) nmax = std::max<long long>(nmax, x->dims[k]);
    // 32-bit element offsets in the workgroup GEMM: the workspace of one train stays below 2^31 doubles
    const long long es = (x->el == 2 || A->el == 2) ? 2 : 1;
    if (rxmax >= (1LL << 31) || rymax >= (1LL << 31) || Rmax >= (1LL << 31) || rxmax * rymax >= (1LL << 31) || rxmax * rymax * Rmax >= (1LL << 31)
        || es * (2 + 2 * nmax) * rxmax * rymax * Rmax >= (1LL << 31))
        return fail(TTN_ERR_UNSUPPORTED, (w + ": ranks too large (the three-layer state of one train reaches 2^31 doubles)").c_str());
    return TTN_OK;
}

// The launches, after braket_check: d_out receives `batch` interleaved (re, im) pairs in device memory.
static int braket_launch(const char* who, ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out) {
    if (x->el == 1 && A->el == 1) {                                      // all Float64: k_expect's number, imaginary part +0.0
        int rc = g_braket_real.ensure(sizeof(double) * x->batch);
        if (rc) return rc;
        if ((rc = sandwich_launch(who, x, A, y, g_braket_real.as<double>()))) return rc;
        hipLaunchKernelGGL(k_braket_widen, dim3((x->batch + 255) / 256), dim3(256), 0, g_stream, g_braket_real.as<double>(), d_out, x->batch);
        HIPCHK(hipGetLastError());
        return TTN_OK;
    }
    const int d = x->d;
    long long rxmax = 1, rymax = 1, Rmax = 1, nmax = 1;
    for (int m = 0; m <= d; ++m) {
        rxmax = std::max<long long>(rxmax, x->bound[m]); rymax = std::max<long long>(rymax, y->bound[m]); Rmax = std::max<long long>(Rmax, A->rks[m]);
    }
    bool qtt = Rmax <= BRAKET_QTT_OPR_MAX;
    for (int k = 0; k < d; ++k) { nmax = std::max<long long>(nmax, x->dims[k]); qtt = qtt && x->dims[k] == 2; }
    // the on-chip kernel takes the trains of its class; the general kernel runs when the batch may hold others (rank bounds above the
    // limit: a ragged batch can still hold trains below it) and, with skip_fit set, leaves alone what the first kernel took
    const bool any_general = !qtt || rxmax > BRAKET_QTT_RMAX || rymax > BRAKET_QTT_RMAX;
    const long long general = any_general ? 2 * (2 + 2 * nmax) * rxmax * rymax * Rmax : 0;
    const long long per_train = std::max<long long>(general, qtt ? 2 * Rmax * BRAKET_IMG : 0) + 16;
    int rc = scratch_take(sizeof(double) * (size_t)per_train * x->batch);
    if (rc) return rc;
    BraketArgs P;
    P.x = x->dev(); P.y = y->dev(); P.A = A->dev();
    P.scratch = g_scratch.as<double>(); P.scratch_stride = per_train;
    P.rxmax = (int)rxmax; P.rymax = (int)rymax; P.Rmax = (int)Rmax; P.nmax = (int)nmax;
    P.skip_fit = qtt ? 1 : 0;
    P.out = d_out;
    const dim3 grid(x->batch), block(TTN_WG);
    const size_t lds = BRAKET_LDS_BYTES(d);
    HIPCHK(hipEventRecord(g_launch_ev0, g_stream));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !qtt : !any_general) continue;
        const int rm = pass == 0 ? (int)Rmax : 0;
        if (x->el == 2 && A->el == 2) braket_dispatch<true, true>(rm, grid, block, lds, P);
        else if (x->el == 2) braket_dispatch<false, true>(rm, grid, block, lds, P);
        else braket_dispatch<true, false>(rm, grid, block, lds, P);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g_launch_ev1, g_stream));
    g_have_launch_ms = true;
    return TTN_OK;
}

int ttn_braket_dev(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !A || !y || !d_out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_braket_dev")) return rb;
    if (int rc = braket_check("ttn_braket_dev", x, A, y)) return rc;
    return braket_launch("ttn_braket_dev", x, A, y, d_out);
}

int ttn_braket(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* out) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    NEED_INIT();
    if (!x || !A || !y || !out) return fail(TTN_ERR_ARG, "null pointer");
    if (int rb = single_op(A, "ttn_braket")) return rb;
    int rc = braket_check("ttn_braket", x, A, y);
    if (rc) return rc;
    rc = g_dout.ensure(sizeof(double) * 2 * x->batch);
    if (rc) return rc;
    if ((rc = braket_launch("ttn_braket", x, A, y, g_dout.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, g_dout.p, sizeof(double) * 2 * x->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_BRAKET_H
