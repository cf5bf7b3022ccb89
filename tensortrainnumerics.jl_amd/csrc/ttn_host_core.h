// ttn_host_core.h — host API, lowest layer: the state every call needs, errors, DevBuf, the handle types, failure codes.
//
// The host API (the C ABI of include/ttn.h) is being cut into csrc/ttn_host_*.h, one header per feature, layered: a header includes the
// lower ones whose helpers or state it uses (an entry point of another feature is called through its declaration in include/, like
// any caller's); ttn_api.hip includes them lowest first, holds the features not cut out yet, and ends with ttn_init / ttn_finalize,
// which see every module's state.  So far, lowest first: _lds, _core, then _dot, _measure, _sample, _handles, _stream, _rect, _compress,
// _braket (above _dot: its all-Float64 form is k_expect's launch), _tangent (above _stream: its coefficients travel in g_grad_coef),
// _contract (on _core alone).
// State that one module alone reads or writes is declared in that module's header; what two modules share stands with the lower of
// them, whose head comment names the other; only what many share stands here.  These headers are included by ttn_api.hip ONLY —
// ttn_wg512.hip never sees one: everything in them has internal linkage (`static`, unnamed namespace) and the library state must
// exist exactly once.  What crosses to ttn_wg512.hip is declared in ttn_wg512.h.
#ifndef TTN_HOST_CORE_H
#define TTN_HOST_CORE_H
#include "../../include/ttn.h"
#include "ttn_common.h"
#include "ttn_rect_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------
// global state
// ------------------------------------------------------------------------------------------------
namespace {
std::set<struct ttn_tt_s*> g_live;  // every live ttn_tt handle (ttn_status_all walks them)
std::recursive_mutex g_mu;
bool g_init = false;
int g_device = -1;
hipStream_t g_stream = nullptr;
hipEvent_t g_launch_ev0 = nullptr, g_launch_ev1 = nullptr;   // the kernels of the last timed launch: dot, orthogonalize, measurements, operator products (ttn_last_launch_ms)
bool g_have_launch_ms = false;
std::string g_err = "";

int fail(int code, const char* what) {
    g_err = what;
    return code;
}
int hipfail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (int)e > 0 ? (int)e : 999;
}
#define HIPCHK(call)                                  \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return hipfail(e_, #call); \
    } while (0)
#define NEED_INIT() \
    if (!g_init) return fail(TTN_ERR_NOT_INIT, "ttn_init has not been called")

// Device memory the library keeps between calls.  ensure() grows it to exactly `n` bytes (after the stream has drained: a launch
// in flight may still read the old allocation) and keeps it when it is already large enough.  Every DevBuf links itself into one list
// as it is constructed (all of them are namespace-scope objects of this translation unit) and ttn_finalize walks that list: a buffer
// declared in any header is released with the rest.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf* next;
    inline static DevBuf* head = nullptr;
    DevBuf() : next(head) { head = this; }
    DevBuf(const DevBuf&) = delete;              // a copy would not be on the list
    DevBuf& operator=(const DevBuf&) = delete;
    int ensure(size_t n) {
        if (n <= bytes) return TTN_OK;
        if (p) { HIPCHK(hipStreamSynchronize(g_stream)); HIPCHK(hipFree(p)); p = nullptr; bytes = 0; }
        HIPCHK(hipMalloc(&p, n));
        bytes = n;
        return TTN_OK;
    }
    void release() { if (p) hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
DevBuf g_scratch;          // per-call workspace of every launch
DevBuf g_dout;             // [batch] doubles: dot results, the factors of ttn_scale_batch
DevBuf g_pending_status;   // one bit per failure code of handles FREED before anybody queried them (ttn_status_all)

// Poison mode (ttn_selftest_poison): a test switch, host side only.  While it is on, the per-call workspace is filled with
// an 8-byte pattern at every acquisition, and new handle arenas and the self-test hooks' allocations are filled with it instead of being
// cleared or left raw — a kernel that reads a byte nobody wrote then computes with the pattern instead of with zeros or plausible stale
// numbers.  Off (the default) it costs one host-side test per acquisition or creation and launches nothing.
bool g_poison = false;
unsigned long long g_poison_pat = 0;
}  // namespace

__global__ void k_poison_fill(unsigned long long* p, size_t n, unsigned long long pat) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = pat;
}
// `bytes` of device memory at p (8-byte aligned) <- the pattern, on the library stream; the up to 7 bytes behind the last whole word: 0xff
static int poison_fill(void* p, size_t bytes) {
    const size_t n = bytes / 8;
    if (n) {
        hipLaunchKernelGGL(k_poison_fill, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, g_stream,
                           static_cast<unsigned long long*>(p), n, g_poison_pat);
        HIPCHK(hipGetLastError());
    }
    if (bytes % 8) HIPCHK(hipMemsetAsync(static_cast<char*>(p) + 8 * n, 0xff, bytes % 8, g_stream));
    return TTN_OK;
}
// The acquisition of the per-call workspace: every entry point that launches on g_scratch takes it here, before its first launch or
// copy into it.  Nothing an earlier call left there may be read afterwards; in poison mode the whole buffer is overwritten to prove it.
static int scratch_take(size_t n) {
    const int rc = g_scratch.ensure(n);
    if (rc || !g_poison) return rc;
    return poison_fill(g_scratch.p, g_scratch.bytes);
}
// There is no non-filling form: no entry point needs workspace contents across a second acquisition today (DESIGN §4.32 lists the
// candidates and why each rebuilds what it reads).  One that does must add such a form here and say what survives it, and why.
// A fresh device allocation of a handle or a self-test hook: the pattern in poison mode, else zeros (`clear`) or left raw
static int fresh_fill(void* p, size_t bytes, bool clear) {
    if (g_poison) return poison_fill(p, bytes);
    if (clear) HIPCHK(hipMemsetAsync(p, 0, bytes, g_stream));
    return TTN_OK;
}

// ------------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------------
struct ttn_tt_s {
    int d = 0, batch = 0;
    int el = 1;                               // doubles per element: 1 Float64, 2 ComplexF64 (interleaved; d_dims then holds 2 n_k, see ttn_cplx_kernels.h)
    std::vector<int64_t> dims, cap, bound;   // bound[m]: host upper bound on the current rank of any train
    std::vector<long long> off;               // d+1 slot offsets
    long long stride = 0;
    double* d_data = nullptr;
    long long* d_off = nullptr;
    long long* d_rks = nullptr;
    long long* d_cap = nullptr;
    int* d_dims = nullptr;
    std::vector<int64_t> ot;                  // [batch][d] host-side gauge flags (never data dependent)
    int* d_status = nullptr;                  // [2][batch]: failure codes of the dense kernels that wrote THIS handle — sticky (kernels only
                                              // store non-zero codes, ttn_compress_status reads and clears) — then the sweep counts of the last launch
    // singular-value capture
    bool sv_on = false;
    double* d_sv = nullptr;
    int sv_steps = 0, sv_pmax = 0;
    TTDev dev() const {
        TTDev t;
        t.data = d_data; t.stride = stride; t.off = d_off; t.rks = d_rks; t.dims = d_dims; t.cap = d_cap;
        t.d = d; t.batch = batch;
        return t;
    }
};
struct ttn_tto_s {
    int d = 0;
    int batch = 1;                            // operators in the handle (include/ttn_opbatch.h): equal dims and ranks, operator b at d_data + b * stride
    long long stride = 0;                     // doubles per operator: off[d]
    int el = 1;                               // 1 Float64, 2 ComplexF64 (slots of twice the doubles; d_dims keeps n_k, d_dims2 holds 2 n_k^2)
    std::vector<int64_t> dims, rks;
    std::vector<long long> off;
    double* d_data = nullptr;
    long long* d_off = nullptr;
    long long* d_rks = nullptr;
    int* d_dims = nullptr;
    int* d_dims2 = nullptr;                   // [d] n_k^2: the dims of the operator seen as a vector (tto_to_ttv)
    std::vector<int64_t> ot;                  // [d] gauge flags (tto_ot; zeros unless ttn_tto_set_ot or an operation sets them)
    TTODev dev() const {
        TTODev t;
        t.data = d_data; t.off = d_off; t.rks = d_rks; t.dims = d_dims; t.d = d;
        t.stride = batch > 1 ? stride : 0;    // 0: every train reads the one operator
        return t;
    }
    // The operator as ONE train of physical dimensions n_k^2 whose capacity is its ranks: an operator core (n, n, r_l, r_r) is byte for
    // byte the vector core (n^2, r_l, r_r), and the 16-byte slot rounding of both handle kinds gives the same offsets.
    TTDev vdev() const {
        TTDev t;
        t.data = d_data; t.stride = off.empty() ? 0 : off.back(); t.off = d_off; t.rks = d_rks; t.dims = d_dims2; t.cap = d_rks;
        t.d = d; t.batch = 1;
        return t;
    }
};

// A rectangular TT operator (include/ttn_rect.h): cores (n_out, n_in, R_l, R_r), Float64, immutable, ranks known on the host.  A type
// of its own: no entry point written for square operators can be handed one.
struct ttn_rtto_s {
    int d = 0;                                // M, the number of sites
    std::vector<int64_t> odims, idims, rks;
    std::vector<int> singles;                 // 0-based sites with n_in == 1 (ttn_apply_rect needs exactly one)
    std::vector<long long> off;
    double* d_data = nullptr;
    long long* d_off = nullptr;
    long long* d_rks = nullptr;
    int* d_dims = nullptr;                    // [2 M]: n_out, then n_in
    RTTODev dev() const {
        RTTODev t;
        t.data = d_data; t.off = d_off; t.rks = d_rks; t.odims = d_dims; t.idims = d_dims + d; t.d = d;
        t.s = singles.empty() ? -1 : singles[0];
        return t;
    }
};

static bool same_dims(const std::vector<int64_t>& a, const std::vector<int64_t>& b) { return a == b; }

// A Float64-only entry point that receives a ComplexF64 handle is refused before any launch: it would read half a slot as a whole one.
static bool any_c64(std::initializer_list<const ttn_tt_s*> tts, std::initializer_list<const ttn_tto_s*> ops = {}) {
    for (const ttn_tt_s* h : tts) if (h && h->el == 2) return true;
    for (const ttn_tto_s* h : ops) if (h && h->el == 2) return true;
    return false;
}
static int refuse_c64(const char* who) {
    g_err = std::string(who) + ": Float64 only, a ComplexF64 handle is not supported";
    return TTN_ERR_UNSUPPORTED;
}
#define F64_ONLY(who, ...) do { if (any_c64(__VA_ARGS__)) return refuse_c64(who); } while (0)
static int refuse_mixed(const char* who) {
    g_err = std::string(who) + ": the element types (Float64 / ComplexF64) of the handles do not fit this call";
    return TTN_ERR_UNSUPPORTED;
}

// An operator batch (include/ttn_opbatch.h) is taken by the entry points listed there; every other one refuses it before any launch: it
// would read operator 0 for every train, or 1 train's worth of a batch of slots.
static int single_op(const ttn_tto_s* A, const char* who) {
    if (!A || A->batch <= 1) return TTN_OK;
    g_err = std::string(who) + ": an operator batch is not supported here (ttn_opbatch.h lists the calls that take one; ttn_tto_select gives one operator of it)";
    return TTN_ERR_UNSUPPORTED;
}
// ... and the ones that take it need one operator per train
static int op_batch_fits(const ttn_tto_s* A, int batch) {
    if (A->batch > 1 && A->batch != batch) { g_err = "batch sizes differ (the operator batch and the trains)"; return TTN_ERR_DIMS; }
    return TTN_OK;
}

// ttn_tt_free / ttn_status_all: bit `code` of the library-level word for every failure code recorded on the handle (which one is
// reported is decided on the host, by the order of status_table)
__global__ void k_fold_status(const int* status, int batch, unsigned* pending) {
    unsigned m = 0;
    for (int b = threadIdx.x; b < batch; b += 64) if (status[b]) m |= 1u << status[b];
    if (m) atomicOr(pending, m);
}

// Owner of a handle that a call builds or only needs until it returns: the destructor frees the handle, with whatever device memory it
// holds by then, on every return path, unless release() has handed it to the caller.
template <class H, int (*Free)(H*)>
struct Owned {
    H* h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { if (h) Free(h); }
    H* release() { H* t = h; h = nullptr; return t; }
};
using OwnedTT = Owned<ttn_tt_s, ttn_tt_free>;
using OwnedTTO = Owned<ttn_tto_s, ttn_tto_free>;
using OwnedRTTO = Owned<ttn_rtto_s, ttn_rtto_free>;

extern "C" {
// ---- failure codes ------------------------------------------------------------------------------------------------
// What each per-train code of the dense kernels (TtnStatus, csrc/ttn_common.h) means to a caller.  The first entry whose code any
// train carries is the one reported.
const struct { int code, err; const char* msg; } status_table[] = {
    {TTN_ST_LANCZOS, TTN_ERR_NO_CONVERGENCE, "a Lanczos local solve exhausted linsolv_maxiter restarts above 1e3 * linsolv_tol"},
    {TTN_ST_NONFINITE, TTN_ERR_NO_CONVERGENCE, "a local eigenvalue or eigenvector was not finite (NaN or Inf in the operator or the start train)"},
    {TTN_ST_SINGULAR, TTN_ERR_SINGULAR, "a local system K is singular (als_linsolve), or a local metric S_s is not positive definite (als_gen_eigsolv)"},
    {TTN_ST_RANKS_DIFFER, TTN_ERR_DIMS, "a train's ranks differ from the ranks the call needs (als_linsolve: the start handle; ttn_apply_pullback: R .* x; ttn_tt_cores_axpby: x; ttn_tangent_project / ttn_tangent_to_tt: U, V and xi)"},
    {TTN_ST_RANK_OVERFLOW, TTN_ERR_CAPACITY, "a rank grew beyond the rank capacity of its handle / working slot (site-swap chain or ttv_decomp)"},
    {TTN_ST_JACOBI, TTN_ERR_NO_CONVERGENCE, "Jacobi SVD hit its sweep limit"},
};

// `seen`: bit c set for every code c recorded (k_fold_status builds the same word on the device).  `who` prefixes the message.
static int status_error(unsigned seen, const char* who = nullptr) {
    for (const auto& s : status_table)
        if (seen & (1u << s.code)) return fail(s.err, who ? (std::string(who) + ": " + s.msg).c_str() : s.msg);
    return TTN_OK;
}

// Failure codes of every dense kernel that wrote `h` since the last call, as bits of one word (synchronises).  The codes are sticky
// on the device — a kernel only ever stores a non-zero code, so a failure inside a chain of launches survives the launches after
// it — and are cleared here, on read.
static int take_status(ttn_tt_t h, unsigned& seen) {
    std::vector<int> st(h->batch);
    HIPCHK(hipMemcpyAsync(st.data(), h->d_status, sizeof(int) * h->batch, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemsetAsync(h->d_status, 0, sizeof(int) * h->batch, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    seen = 0;
    for (int c : st) if (c) seen |= 1u << c;
    return TTN_OK;
}
}  // extern "C"
#endif  // TTN_HOST_CORE_H
