/*
 * ttn.h — C ABI of the MI355X-native TT/QTT core-arithmetic backend ("libttn_hip.so").
 *
 * This is the drop-in boundary for ONE hot path of TensorTrainNumerics.jl v1.1.3: TT-operator
 * apply, TT dot / hadamard / + / scalar*, orthogonalize and the tt_compress! rounding sweep.  The
 * reference has no FFI of its own (it is pure Julia; L1 is reached by multiple dispatch), so every
 * entry point below cites the Julia method it replaces; the Julia-side `ccall` binding a maintainer
 * would add is shown in INTEGRATION.md and julia/TTNBackend.jl.
 *
 * Conventions
 *   - plain C, no C++/torch types; all integers are int64_t, all payload is double (fp64; ComplexF64 handles: interleaved
 *     (re, im) pairs of doubles, see "ComplexF64 trains and operators" below);
 *   - arrays are COLUMN-MAJOR exactly as the reference stores them:
 *       vector core  k : (n_k, r_{k-1}, r_k)            offset i + n*(a + r_{k-1}*b)
 *       operator core k: (n_k, n_k, R_{k-1}, R_k)       offset i + n*(j + n*(a + R_{k-1}*b))
 *     (src/tt_tools.jl:23-29, :48-54); rank vectors have length d+1, `ot` vectors length d;
 *   - site numbers (`k`, `center`) are 1-based like the reference;
 *   - every function returns int: 0 = ok, <0 = argument error (the Julia shim maps these to the
 *     AssertionError the reference throws), >0 = HIP runtime error (hipError_t value).
 *     Functions never throw and never abort.  ttn_last_error_string() describes the last failure.
 *   - the library is usable from any host thread; calls are serialised internally on one HIP stream.
 */
#ifndef TTN_H
#define TTN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (negative = argument errors, mirrored as AssertionError on the host side) ---- */
#define TTN_OK                 0
#define TTN_ERR_DIMS          -1   /* "Incompatible dimensions"  (tt_operations.jl:11,102,240,344) */
#define TTN_ERR_BOND_INDEX    -2   /* "k must be in 1:(N-1)"     (tt_tools.jl:744)                  */
#define TTN_ERR_SWEEPS        -3   /* "sweeps must be >= 1"      (tt_tools.jl:773)                  */
#define TTN_ERR_CENTER        -4   /* "Impossible orthogonalization" (tt_tools.jl:513)              */
#define TTN_ERR_CAPACITY      -5   /* destination handle too small for the result ranks             */
#define TTN_ERR_ARG           -6   /* null pointer / non-positive size / bad handle                 */
#define TTN_ERR_NOT_INIT      -7   /* ttn_init was not called (or failed)                           */
#define TTN_ERR_UNSUPPORTED   -8   /* shape outside what the kernels support (stated in DESIGN.md)  */
#define TTN_ERR_NO_CONVERGENCE -9  /* Jacobi SVD hit its sweep limit on some bond                   */
#define TTN_ERR_SINGULAR      -10  /* als_linsolve: a local system K is singular (LAPACK's SingularException)  */

/* ---- library lifetime ------------------------------------------------------------------------ */
int         ttn_init(int device);            /* binds to HIP device `device`, creates the stream   */
int         ttn_finalize(void);
const char* ttn_version(void);
const char* ttn_last_error_string(void);
int         ttn_sync(void);                  /* hipStreamSynchronize on the library stream          */
int         ttn_device_count(int* n);        /* hipGetDeviceCount (does not initialise a device)    */

/* ---- device-resident handles ------------------------------------------------------------------
 * A ttn_tt is a BATCH of `batch` TT vectors with common d/dims and a common per-bond rank CAPACITY;
 * each train carries its own current ranks (they live on the device because tt_compress! makes them
 * data dependent).  One contiguous fp64 arena: train b, core k at  data + b*stride + off[k].
 * A ttn_tto is one TT operator shared by every train of a batch.
 * Replaces: TTvector / TToperator containers (src/tt_tools.jl:23-29, :48-54).
 */
typedef struct ttn_tt_s*  ttn_tt_t;
typedef struct ttn_tto_s* ttn_tto_t;

int ttn_tt_create(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out);
int ttn_tt_free(ttn_tt_t h);
/* cores[k] points at n_k*rks[k]*rks[k+1] doubles (host memory, column-major) */
int ttn_tt_upload(ttn_tt_t h, int64_t b, const double* const* cores, const int64_t* rks, const int64_t* ot);
/* copies train `src_b` (cores + ranks + ot) over every other train of the batch, on the device */
int ttn_tt_replicate(ttn_tt_t h, int64_t src_b);
/* current ranks / ot flags of train b (synchronises the stream) */
int ttn_tt_ranks(ttn_tt_t h, int64_t b, int64_t* rks, int64_t* ot);
/* bound[m] = max over the trains of the CURRENT rank of bond m (synchronises); also tightens the host-side rank
 * bounds the capacity checks of the other calls use (they only know upper bounds after data-dependent truncations) */
int ttn_tt_max_ranks(ttn_tt_t h, int64_t* bound);
/* cores[k] must have room for n_k*rks[k]*rks[k+1] doubles with the CURRENT ranks (see ttn_tt_ranks) */
int ttn_tt_download(ttn_tt_t h, int64_t b, double* const* cores);
int ttn_tt_batch(ttn_tt_t h, int64_t* batch);
/* device copy dst <- src (same d/dims, dst capacity >= src current ranks) */
int ttn_tt_copy(ttn_tt_t dst, ttn_tt_t src);

int ttn_tto_create(int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores, ttn_tto_t* out);
int ttn_tto_free(ttn_tto_t h);

/* ---- the hot path on handles (every op runs on all trains of the batch, asynchronously) -------- */

/* y = A * x       replaces *(A::TToperator, v::TTvector), src/tt_operations.jl:101-111 */
int ttn_apply(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y);

/* tt_compress!(psi, max_bond; truncerr, sweeps)   src/tt_tools.jl:772-789 (+ :743-768 per bond and the
 * effective _svdtrunc, src/tt_cross_interpolation.jl:149-166).  The reference's trailing
 * `orthogonalize(psi; i=k)` (:769) is not computed: tt_compress! discards its value (:779,:785). */
int ttn_compress(ttn_tt_t psi, int64_t max_bond, double truncerr, int64_t sweeps);

/* Device-side status of the handle (synchronises).  Every call that runs bond steps or local solves on psi — ttn_compress,
 * ttn_apply_compress, ttn_bond_truncate, ttn_sweep, ttn_apply_sweep, ttn_swap_sites, ttn_hadamard_ttm, ttn_ttv_decomp,
 * ttn_tt_split_sites, ttn_tt_merge_sites, the linear solvers — records per train the FIRST condition its kernels meet:
 * TTN_ERR_CAPACITY (a rank outgrew its slot), TTN_ERR_NO_CONVERGENCE (a Jacobi SVD / eigensolver hit its sweep limit),
 * TTN_ERR_SINGULAR (singular local system).  The record is
 * STICKY per handle: it survives later calls and is returned — and cleared — by this query, so a chain of asynchronous calls needs
 * one query at its end.  If non-null, total_jacobi_sweeps[b] receives the number of Jacobi sweeps train b used in the last call
 * (diagnostics). */
int ttn_compress_status(ttn_tt_t psi, int64_t* total_jacobi_sweeps);
/* One query for a whole chain (synchronises once): the most severe failure code recorded on ANY live handle (left in place
 * there: ttn_compress_status of that handle still reports and clears it) or on a handle that was FREED before anybody queried it
 * (ttn_tt_free folds an unread code into a library-level word, cleared here).  Most severe, here and wherever codes of several
 * trains meet: Lanczos exhaustion, then a non-finite local eigenpair, a singular local system, ranks that differ from the start
 * handle, a rank that outgrew its slot, a Jacobi sweep limit.  A device-resident chain that creates and frees
 * temporaries (RK4 stages, Krylov vectors) needs this once per time step / iteration instead of one query per compress. */
int ttn_status_all(void);

/* Rank bounds of tt_compress! (k = 0) or one _tt_bond_truncate! (k = 1-based bond).  The reference keeps
 * r = min(length(s), max_bond) singular values (tt_cross_interpolation.jl:152,164), so the rank of a rank-deficient
 * bond can GROW up to min(n_k r_{k-1}, n_{k+1} r_{k+1}, max_bond).  need[m] >= rks[m] is the capacity a handle / a
 * host buffer must have for bond m; fin[m] bounds the ranks after the call.  Either output may be null. */
int ttn_compress_rank_bound(int64_t d, const int64_t* dims, const int64_t* rks, int64_t max_bond, int64_t sweeps, int64_t k,
                            int64_t* need, int64_t* fin);

/* _tt_bond_truncate!(psi, k; max_bond, truncerr) without the discarded orthogonalize; k is 1-based */
int ttn_bond_truncate(ttn_tt_t psi, int64_t k, int64_t max_bond, double truncerr);

/* --- core-wise sharded chains (one segment of the chain per GPU, boundary-core hand-offs between neighbours).
 * A segment is an ordinary handle whose boundary ranks need not be 1.
 * ttn_sweep: the bond steps of src/tt_tools.jl:780-785 restricted to one direction over the bonds k_first .. k_last
 * (1-based like ttn_bond_truncate; descending when k_first > k_last).
 * ttn_tt_core_extent / _export / _import: move core k (1-based) of every train to / from a dense device buffer
 * [batch][dims[k]*bound_left*bound_right] plus its two ranks [batch][2] (device pointers, e.g. of the tensor handed to
 * ncclSend/ncclRecv); import sets the host-side rank bounds the sender reports. */
int ttn_sweep(ttn_tt_t psi, int64_t k_first, int64_t k_last, int64_t max_bond, double truncerr);
/* The fused form for a segment: ttn_apply_begin gives y the ranks of A*x (no core is written); a boundary core may then be imported
 * into y (ttn_tt_core_import); ttn_apply_sweep runs ONE L->R pass over the bonds k_first <= ... <= k_last with the cores right of
 * the moving front still virtual (built from A and x inside the bond step, like ttn_apply_compress) — every core of the range is
 * real afterwards.  first_core_real != 0: core k_first was imported and is used as it is; 0: it is written out first.
 * ttn_stream_handle: the hipStream_t all calls are enqueued on, for event-based ordering against the caller's own streams. */
int ttn_apply_begin(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y);
int ttn_apply_sweep(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y, int64_t k_first, int64_t k_last, int64_t max_bond, double truncerr, int first_core_real);
int ttn_stream_handle(void** stream);
int ttn_tt_core_extent(ttn_tt_t h, int64_t k, int64_t* doubles_per_train, int64_t* bound_left, int64_t* bound_right);
int ttn_tt_core_export(ttn_tt_t h, int64_t k, double* dev_buf, int64_t* dev_rks2);
int ttn_tt_core_import(ttn_tt_t h, int64_t k, const double* dev_buf, const int64_t* dev_rks2, int64_t bound_left, int64_t bound_right);

/* --- site-swap chains: the two-site SVD step with the physical indices of the two cores exchanged
 * (_ttm_swap!, src/tt_operations.jl:365-382; _swap_adjacent_sites, src/qtt_tools.jl:660-695): factors U and S*Vt.
 * All physical dimensions of the train must be equal (QTT: 2) and n * rank capacity <= 256.
 * ttn_hadamard_ttm: z = hadamard_ttm(x, y; tol, rmax) (src/tt_operations.jl:398-422; d(d-1)/2 swaps + d site-wise
 *   contractions, rank rule = the relative tail norm of tt_cross_interpolation.jl:149-166).  work_cap = rank capacity of the
 *   2d working slots; a rank above it (or above z's capacity) is reported by ttn_compress_status as TTN_ERR_CAPACITY.
 * ttn_swap_sites: the swap list of reorder (src/qtt_tools.jl:763-769) in place; swaps[i] = k (1-based) exchanges sites
 *   k and k+1; rank rule = count(s > threshold * s[1]) (at least 1), or every singular value when threshold == 0. */
int ttn_hadamard_ttm(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z, double tol, int64_t rmax, int64_t work_cap);
int ttn_swap_sites(ttn_tt_t x, int64_t nswaps, const int64_t* swaps, double threshold);

/* z_b = ttv_decomp(tensor_b; index, tol) (src/tt_tools.jl:186-252): hierarchical SVD of `batch` dense tensors of shape
 * z.dims (HOST memory, [batch][prod(dims)], column-major like a Julia Array), root at site `index` (1-based), singular values
 * below `tol` discarded (absolute).  Ranks are bounded by the handle's capacity: a larger rank is reported by
 * ttn_compress_status as TTN_ERR_CAPACITY.  Sets the orthogonality flags -1 / 0 / +1 like the reference.  Synchronises. */
int ttn_ttv_decomp(ttn_tt_t z, const double* tensors, int64_t index, double tol);
/* ttn_ttv_decomp with the tensors already in DEVICE memory ([batch][prod(dims)], on the library's stream): the same kernel on the
 * same data, without the host -> device copy.  The input buffer is only read.  Limits, status reporting and the orthogonality flags are
 * those of ttn_ttv_decomp.  Synchronises. */
int ttn_ttv_decomp_dev(ttn_tt_t z, const double* d_tensors, int64_t index, double tol);

/* --- split and merge sites (csrc/ttn_resite_kernels.h; to_qtt / to_ttv, src/qtt_tools.jl:254-360), Float64 only.  z is
 * created by the caller with the new dims and a rank capacity (the ttn_tt_kron convention), has x's batch and must not be x.
 * Both calls are asynchronous on the library's stream, read x's device-resident per-train ranks, write z's ranks per train
 * and clear z's orthogonality flags; a rank above z's capacity is that train's TTN_ERR_CAPACITY through
 * ttn_compress_status(z).
 * ttn_tt_split_sites: z_b = to_qtt(x_b, split_dims; threshold).  nsplit[i] factors for site i of x, the factors of all sites
 *   one after the other in split_dims (sum(nsplit) entries, the FIRST factor of a site its most significant digit); z.dims
 *   must be exactly split_dims.  Every factor but a site's last costs one SVD of the (r_prev s) x (rest r_next) unfolding:
 *   the new core is U, S V' is carried on.  Rank rule of ttn_swap_sites: every singular value when threshold == 0, else
 *   count(s > threshold * s[1]), at least 1 (an all-zero unfolding keeps one zero direction where the reference would keep
 *   none).
 * ttn_tt_merge_sites: z_b = to_ttv(x_b, merge_numbers).  Site g of z is the product of merge_numbers[g] consecutive cores of
 *   x with the physical indices merged big-endian (i1 n2 + i2); no SVD, the ranks are x's at the kept bonds.
 * Refused before any launch, with a message that names the call.  TTN_ERR_ARG: a null pointer, x == z, sum(nsplit) != z's
 * sites, sum(merge_numbers) != x's sites, ngroups != z's sites, a factor list whose product differs from the site's
 * dimension, z.dims that differ from the flattened split lists / the merged products, differing batches, threshold < 0.
 * TTN_ERR_CAPACITY: z's capacity at a bond kept from x below x's rank bound.  TTN_ERR_UNSUPPORTED: a ComplexF64 handle; a
 * split unfolding with a short side above 4096 or more than 2^27 entries (ranks bounded by x's rank bound and z's capacity,
 * as in ttn_ttv_decomp); more than 64 sites in x for a split; for a merge a batch above 65535, a merged dimension of 2^31 or
 * more, or 2^31 output tiles in one core. */
int ttn_tt_split_sites(ttn_tt_t x, ttn_tt_t z, const int64_t* nsplit, const int64_t* split_dims, double threshold);
int ttn_tt_merge_sites(ttn_tt_t x, ttn_tt_t z, const int64_t* merge_numbers, int64_t ngroups);

/* --- trains -> dense tensors and QTT grids on the device (csrc/ttn_grid_kernels.h), Float64 only (a ComplexF64 handle:
 * TTN_ERR_UNSUPPORTED before any launch).
 * ttn_tt_to_dense: for every train b of the batch d_out[b * total + sum_k (i_k - 1) strides[k]] = x_b(i_1..i_N); d_out is DEVICE
 *   memory of batch * total doubles, total = prod(dims).  strides == NULL: Julia column-major, i.e. ttv_to_tensor
 *   (src/tt_tools.jl).  The (stride, n) pairs sorted by stride must form a mixed-radix system (the smallest stride is 1, each next
 *   one is the previous stride times that site's n; sites with n = 1 are ignored), which makes the map a bijection onto [0, total):
 *   otherwise TTN_ERR_ARG before any launch.  Limits: total <= 2^27 per train, at most 64 sites, every n <= 4096, end ranks 1 (TTN_ERR_UNSUPPORTED).
 *   The train is cut where both partial products are about sqrt(total) wide; out = L R by fp64 MFMA, stored in output-address
 *   order.  Asynchronous on the library's stream.
 * ttn_qtt_grid_points: coordinates of the entries first .. first + count - 1 of the (2, ..., 2) tensor of a QTT with n_dims * bits
 *   sites (linear index, site 1 fastest), d_X (DEVICE) laid out (n_dims, count).  Bit -> (dim, level): src/qtt_tools.jl:820-829
 *   (interleaved != 0: site = level * n_dims + dim; serial: site = dim * bits + level); grid index g = sum bit * 2^(bits-1-level),
 *   coord = a + g * h, h = (b - a) / (2^bits - 1) computed on the host, one rounded multiply and one rounded add on the device (no
 *   FMA).  Limits: bits <= 52, n_dims * bits <= 62 (TTN_ERR_ARG).  Asynchronous. */
int ttn_tt_to_dense(ttn_tt_t x, const int64_t* strides, double* d_out);
int ttn_qtt_grid_points(int64_t n_dims, int64_t bits, int interleaved, double a, double b, int64_t first, int64_t count, double* d_X);

/* --- als_linsolve(A, b, tt_start; sweep_count) (src/solvers/als.jl:161-222): x = the ALS iterate after
 * sweep_count half sweeps, for every train of the batch (one operator, `batch` right-hand sides b and start trains x0).
 * x receives orthogonalize(x0) first (als.jl:174) and keeps x0's ranks (als.jl:177); the local systems are assembled
 * densely and solved by LU with partial pivoting like the reference's `K \ Pb` (als.jl:58-70).  All trains of x0 must carry
 * the same ranks.  Local systems of up to 2048 unknowns (n r_{i-1} r_i: ranks up to 32 for n = 2) run as ONE persistent launch, one
 * workgroup per train; larger ones — up to 65 536 unknowns; BASELINE config C5 names ranks up to 128 = 32 768 unknowns, an 8.6 GB K —
 * run in the GRID form: assembly and the blocked LU on the whole chip, the half sweeps walked by the host, one train after the other
 * (csrc/ttn_als_grid.h).  ttn_compress_status(x) reports a singular local system (TTN_ERR_SINGULAR). */
int ttn_als_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, int64_t sweep_count);

/* mals_linsolve(A, b, tt_start; tol, rmax) (src/solvers/mals.jl:240-312): one forward and one backward half sweep of
 * two-site solves, ranks adapted by the truncated SVD of every local solution (sv_trunc, clamped to rmax).  x receives
 * orthogonalize(x0) first; x's CAPACITY bounds the ranks (a larger rank: TTN_ERR_CAPACITY through ttn_compress_status) and
 * must keep every two-site system n_i cap_i n_{i+1} cap_{i+2} <= 2048.  The local systems are solved as the reference's
 * `Hermitian(K) \ b` (mals.jl:156,167): the matrix is K's UPPER TRIANGLE mirrored, in the reference's ordering of the unknowns, then LU
 * with partial pivoting.  For a symmetric A that is K; for a non-symmetric A it is not, and the result is the reference's, not the
 * Galerkin solution. */
int ttn_mals_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t rmax);

/* dmrg_linsolve(A, b, tt_start; N = 2, tol, sweep_schedule, rmax_schedule) (src/solvers/dmrg.jl:388-472): two-site sweeps
 * (windows 1..d-2 forward with right_core_move!, d-1..2 backward with left_core_move!, dmrg.jl:187-232) walked through the
 * reference's stage schedule — sweep s ends stage j when s == sweep_schedule[j], the sweep that would end the last stage is
 * the closing solve at window 1 — with the ranks cut by cut_off_index (dmrg.jl:179-185) clamped to the stage's rmax.
 * Local systems up to 2048 unknowns are assembled densely and solved by LU (the reference's `K_full` + `Hermitian(K) \ Pb` branch,
 * dmrg.jl:53-62, :173-175: the upper triangle of K mirrored, in the reference's ordering (r_l, n_i n_{i+1}, r_r) of the unknowns), larger
 * ones matrix-free by conjugate gradients on 1/2 (K + K^T) (see ttn_dmrg_linsolve_it).  For a non-symmetric A the two branches solve
 * different systems, as in the reference.  sweep_schedule must be positive and
 * strictly increasing (anything else does not terminate in the reference); at most 32 full sweeps per call.  Capacity and
 * status as for ttn_mals_linsolve.  N = 1 is ttn_als_linsolve's territory and not offered here. */
int ttn_dmrg_linsolve(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                      const int64_t* rmax_schedule);

/* The same with the reference's local-solver keywords (dmrg.jl:392-396, :92-97): every local system with `it_solver != 0` or with
 * more than `itslv_thresh` unknowns is solved MATRIX-FREE by conjugate gradients on the symmetrised local operator (dmrg.jl:99-171:
 * the three-tensor sandwich G (x) Amid (x) H as fp64 MFMA GEMMs; KrylovKit's `linsolve(...; issymmetric, isposdef, tol, maxiter)`):
 * start vector = the current two-site block, stop at ||residual||_2 < linsolv_tol (absolute) or after linsolv_maxiter iterations.
 * The reference's defaults are it_solver = 1, linsolv_maxiter = 200, linsolv_tol = max(sqrt(tol), 1e-8), itslv_thresh = 256.
 * Dense systems are limited to 2048 unknowns; anything larger is solved matrix-free whatever the keywords say, so two-site
 * systems up to n_i cap_i = n_{i+1} cap_{i+2} = 256 (ranks 128 for n = 2: 65 536 unknowns, BASELINE config C5) are in reach.
 * ttn_dmrg_linsolve itself = it_solver 0, itslv_thresh 2048.  ttn_dmrg_cg_iterations: CG iterations per train of the last call. */
int ttn_dmrg_linsolve_it(ttn_tto_t A, ttn_tt_t b, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                         const int64_t* rmax_schedule, int it_solver, int64_t linsolv_maxiter, double linsolv_tol, int64_t itslv_thresh);
int ttn_dmrg_cg_iterations(int64_t batch, int64_t* iters);

/* dmrg_eigsolve(A, tt_start; N = 2, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
 * (src/solvers/dmrg.jl:501-578) and mals_eigsolve (src/solvers/mals.jl:335-425): the smallest eigenvalue of a real symmetric A and its
 * eigenvector, by two-site sweeps with the walk, rank rules (cut_off_index / sv_trunc, clamped to the stage's rmax) and stage schedule
 * of ttn_dmrg_linsolve; MALS takes the same per-sweep rmax plan (mals.jl:393, :413).  x receives orthogonalize(x0) first and leaves
 * normalised, with the gauge flags the reference leaves.  Per train and micro-step: E[b * hist_len + t] = the local eigenvalue,
 * r_hist[b * hist_len + t] = max(ttv_rks) after the micro-step's core move — the closing DMRG solve records both before its left move
 * (dmrg.jl:539-540).  hist_len must equal ttn_eigsolve_history_len(mode = 1 DMRG / 0 MALS): 2 (d - 2) nsweeps + 1 for DMRG,
 * 2 (d - 1) nsweeps for MALS, nsweeps = the full sweeps of the schedule; anything else is TTN_ERR_ARG.
 * Local problem: the smallest eigenpair of 1/2 (K + K^T).  Dense (Householder tridiagonalisation, Sturm multisection, inverse
 * iteration: |lambda - lambda_LAPACK| ~ 1e-15 ||K||) unless it_solver != 0 or it has more than the threshold unknowns (or more than
 * 2048); then matrix-free thick-restart Lanczos, Krylov dimension 30, full reorthogonalisation, at most linsolv_maxiter restarts,
 * stopped at a Ritz residual <= linsolv_tol.  The threshold is itslv_thresh for DMRG; mals_eigsolve does not forward itslv_thresh to
 * its local solver in the reference (mals.jl:383-390, :403-410), so it is 256 there whatever is passed.  The reference's iterative
 * solvers (KrylovKit eigsolve for DMRG, IterativeSolvers lobpcg for MALS) reach the same eigenpair to linsolv_tol, not the same bits.
 * Every local eigenvector is signed so that its first entry of largest modulus is positive: a batch gives the trains of single calls.
 * Refused before any launch: bad schedules (as ttn_dmrg_linsolve), n_i cap_i above 256, two-site problems above 65 536 unknowns, and a
 * capacity / batch whose workspace — G and H slots, dense K of up to min(N, threshold)^2, Lanczos basis (30 + 1 + 10 + R_max) N_max —
 * does not fit in device memory (TTN_ERR_CAPACITY).  A Lanczos solve that exhausts its restarts with a residual above
 * 1e3 linsolv_tol: TTN_ERR_NO_CONVERGENCE (below that the current Ritz pair is kept, as KrylovKit does).  Synchronises. */
int ttn_dmrg_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                      const int64_t* rmax_schedule, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                      int64_t hist_len, double* E, int64_t* r_hist);
int ttn_mals_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, double tol, int64_t n_stages, const int64_t* sweep_schedule,
                      const int64_t* rmax_schedule, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                      int64_t hist_len, double* E, int64_t* r_hist);
int ttn_eigsolve_history_len(int mode, int64_t d, int64_t n_stages, const int64_t* sweep_schedule, int64_t* len);   /* mode 2: ALS */
/* als_eigsolve(A, tt_start; sweep_schedule, rmax_schedule, noise_schedule, it_solver, itslv_thresh, maxiter, linsolv_tol)
 * (src/solvers/als.jl:251-326) and als_gen_eigsolv(A, S, tt_start; sweep_schedule, rmax_schedule, it_solver, itslv_thresh)
 * (src/solvers/als.jl:344-426): the smallest eigenvalue of a real symmetric A (of the pencil A x = lambda S x, S symmetric positive
 * definite) and its eigenvector, by one-site sweeps at the fixed ranks of each stage.  x receives orthogonalize(x0) first; stage j > 0
 * starts with increase_ranks(x, rmax_schedule[j]; noise = noise_schedule[j]) and orthogonalize, and the environments are rebuilt from
 * the new train (for als_gen_eigsolv too: the reference zero-pads its stale right environments there).  E[b * hist_len + t] = the local
 * eigenvalue of micro-step t; hist_len must equal ttn_eigsolve_history_len(mode = 2) = 2 (d - 1) (sweep_schedule[end] - 1).
 * Local problem: the smallest eigenpair of K_s = 1/2 (K + K^T) (and of the pencil (K_s, S_s)).  Standard: dense (Householder, Sturm
 * multisection, inverse iteration) unless the local size N = n_i r_{i-1} r_i is above 2048 or (it_solver and N > itslv_thresh), then
 * thick-restart Lanczos from the current core, at most maxiter restarts, stopped at a Ritz residual <= linsolv_tol.  Generalized: dense
 * (blocked Cholesky S_s = L L^T, the smallest pair of L^-1 K_s L^-T, x = L^-T y) when !it_solver and N <= min(itslv_thresh, 2048),
 * otherwise LOBPCG with block size 1, no preconditioner, tol 1e-8, at most 500 iterations; the local vector leaves S-normalised.
 * Every local eigenvector is signed so that its first entry of largest modulus is positive: a batch gives the trains of single calls.
 * Noise blocks (noise_schedule null: none) are orthonormal blocks from a counter-based stream keyed by (seed, site, entry), scaled by
 * the noise; noise = 0 pads with exact zeros.
 * Refused before any launch: bad schedules (TTN_ERR_ARG, as ttn_dmrg_eigsolve), a stage rmax not above the maximum rank before it
 * (TTN_ERR_ARG), d < 2, start ranks beyond what orthogonalize keeps, cores too flat for the QR core moves, local sizes above 65 536
 * (TTN_ERR_UNSUPPORTED), a capacity of x below the ranks of a stage or a workspace that does not fit (TTN_ERR_CAPACITY).  Per train: a
 * Lanczos / LOBPCG solve that ends with a residual above 1e3 tol: TTN_ERR_NO_CONVERGENCE; a non-finite local pair: the same, and the
 * train stops; a local metric that is not positive definite: TTN_ERR_SINGULAR, and the train stops.  Operator applications and the
 * largest final residual go to ttn_eigsolve_stats.  Synchronises. */
int ttn_als_eigsolve(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                     const double* noise_schedule, int64_t seed, int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                     int64_t hist_len, double* E);
int ttn_als_gen_eigsolve(ttn_tto_t A, ttn_tto_t S, ttn_tt_t x0, ttn_tt_t x, int64_t n_stages, const int64_t* sweep_schedule,
                         const int64_t* rmax_schedule, int it_solver, int64_t itslv_thresh, int64_t hist_len, double* E);
/* Per train of the last eigensolve: operator applications of its Lanczos solves (0: every local problem dense) and the largest final
 * Lanczos residual norm. */
int ttn_eigsolve_stats(int64_t batch, int64_t* lanczos_applies, double* lanczos_residual);

/* --- TDVP local contractions (src/solvers/tdvp.jl:29-43, :205-208), batched, Float64 (cplx = 0) or ComplexF64
 * (cplx = 1: interleaved re/im pairs, as Julia stores them).  Tensors are column-major in the layouts tdvp1sweep! / tdvp2sweep! hold
 * them in — sites (l, s, r) = permutedims(ttv_vec[k], (2,1,3)), operator cores (a, s, b, s') = permutedims(tto_vec[k], (3,1,4,2))
 * (:52-53) — `batch` of each back to back; the operator core(s) may be one shared tensor (m_shared != 0).
 *   _applyH1_lsr      HAC[α,s,β]      = FL[α,a,α'] AC[α',s',β'] M[a,s,b,s'] FR[β',b,β]             FL (Dl,a,Dl)  AC (Dl,d,Dr)  M (a,d,b,d)  FR (Dr,b,Dr)
 *   _applyH0          HC[α,β]         = FL[α,a,α'] C[α',β'] FR[β',a,β]                             FL (Dl,a,Dl)  C (Dl,Dr)     FR (Dr,a,Dr)
 *   _update_left_env  FLnext[α,a,β]   = FL[α',a',β'] A[β',s',β] M[a',s,a,s'] conj(A[α',s,α])       A (Dl,d,Dr)  M (a_in,d,a_out,d)  FL (Dl,a_in,Dl) -> (Dr,a_out,Dr)
 *   _update_right_env FRprev[α,a,β]   = A[α,s',α'] FR[α',a',β'] M[a,s,a',s'] conj(A[β,s,β'])       A (Dl,d,Dr)  M (a_out,d,a_in,d)  FR (Dr,a_in,Dr) -> (Dl,a_out,Dl)
 *   _applyH2_lsr      HAAC[α,s1,s2,β] = FL[α,a,α'] AAC[α',s1',s2',β'] M1[a,s1,b,s1'] M2[b,s2,c,s2'] FR[β',c,β]
 * Each is a chain of fp64 MFMA GEMMs over strided views of the arrays as they lie (no permuted copies); a complex product is four
 * real ones.  The first five take DEVICE pointers (asynchronous on the library stream); ttn_tdvp_contract_f64 stages HOST arrays:
 * op = 0 applyH1, 1 applyH0, 2 update_left_env, 3 update_right_env, 4 applyH2; dims7 = {Dl, d (d1), Dr, a, b, c, d2} with a = a_in,
 * b = a_out for the environment updates; FL / FR / M1 / M2 that an op does not use are ignored (may be null); X = AC / C / A / AAC. */
int ttn_tdvp_apply_h1(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a, int64_t b, const double* FL, const double* AC,
                      const double* M, const double* FR, double* HAC, int m_shared);
int ttn_tdvp_apply_h0(int cplx, int64_t batch, int64_t Dl, int64_t Dr, int64_t a, const double* FL, const double* C, const double* FR, double* HC);
int ttn_tdvp_update_left_env(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a_in, int64_t a_out, const double* A, const double* M,
                             const double* FL, double* FLnext, int m_shared);
int ttn_tdvp_update_right_env(int cplx, int64_t batch, int64_t Dl, int64_t d, int64_t Dr, int64_t a_out, int64_t a_in, const double* A, const double* M,
                              const double* FR, double* FRprev, int m_shared);
int ttn_tdvp_apply_h2(int cplx, int64_t batch, int64_t Dl, int64_t d1, int64_t d2, int64_t Dr, int64_t a, int64_t b, int64_t c, const double* FL,
                      const double* AAC, const double* M1, const double* M2, const double* FR, double* HAAC, int m_shared);
int ttn_tdvp_contract_f64(int op, int cplx, int64_t batch, const int64_t* dims7, const double* FL, const double* FR, const double* X, const double* M1,
                          const double* M2, double* out, int m_shared);

/* --- dense moves of the TDVP sweeps on one local matrix (src/solvers/tdvp.jl:76-80, :120-126: qr(Aqr), qr(A'); :252, :276: the svd inside
 * _svdtrunc), Float64 (cplx = 0) or ComplexF64 (cplx = 1, interleaved), column-major, DEVICE pointers, the library's stream.
 * ttn_dense_qr: Householder as LAPACK's geqr2 + org2r: A (m x n, overwritten) -> Q (m x r), R (r x n), r = min(m, n); asynchronous.
 * ttn_dense_svd: one-sided Jacobi, m >= n (pass the conjugate transpose otherwise): A (overwritten) -> U (m x n), s (n, descending),
 * Vh (n x n), A = U diag(s) Vh; synchronises (the caller reads s to choose the rank); TTN_ERR_NO_CONVERGENCE after 60 sweeps.
 * LAPACK's contract holds also where s has zeros: U has orthonormal columns and Vh orthonormal rows (U^H U = Vh Vh^H = I, n x n); the
 * columns of U for singular values <= eps s_0 are completed to an orthonormal set (Gram-Schmidt, deterministic). */
int ttn_dense_qr(int cplx, int64_t m, int64_t n, double* A, double* Q, double* R);
int ttn_dense_svd(int cplx, int64_t m, int64_t n, double* A, double* U, double* s, double* Vh);

/* --- TT-cross interpolation (src/tt_cross_interpolation.jl: tt_cross, tt_integrate), csrc/ttn_cross_kernels.h.  DEVICE pointers, the
 * library's stream, Float64 (cplx = 0) or ComplexF64 (cplx = 1, interleaved), column-major matrices, int64 indices 1-based.
 * ttn_cross_maxvol: maxvol!(A, tol, maxiter) on one m x r matrix, r <= m: initial rows by LU with partial pivoting (getrf's choice),
 *   then swaps at the largest |C_ij| (ties: the smallest column-major index) while it exceeds tol, at most maxiter of them, C kept by
 *   Sherman-Morrison updates.  piv (r): the pivot rows in column order; C (m x r) = A / A[piv,:] computed again from scratch (LU solve
 *   with the r x r block).  dinfo (device, 2 words; may be null: library memory) receives {0 or TTN_ERR_SINGULAR, swaps}; with a
 *   HOST hinfo the call synchronises, copies them there and returns TTN_ERR_SINGULAR on a zero pivot; without it the call is
 *   asynchronous.  piv always holds rows of A.  Limits: r <= 1024, m <= 2^20 (TTN_ERR_UNSUPPORTED before any launch).
 * ttn_cross_points: the P x N index matrix of a fibre (mode 0: _build_fiber_indices of site `site`, i fastest, then r_left, then
 *   r_right; L rl x (site-1), R rr x (N-site)), of a superblock (mode 1: _sample_superblock of sites site, site+1, r_l fastest, then
 *   i1, i2, r_g; L rl x (site-1), R rr x (N-site-1)) or a given one (mode 2: idx_in); into idx_out and / or the coordinates X (P x N)
 *   gathered from the domain arrays concatenated in dom at offsets doff (N + 1, device); asynchronous.
 * ttn_cross_eval: _evaluate_tt (idx, P x N) or _contract_with_weights (w: the weight vectors concatenated, P = 1) of the train whose
 *   cores (n_k x r_{k-1} x r_k, device pointers in a HOST array) and dims / ranks (HOST) are given, ranks <= 1024; out (P).  With
 *   yref, err[0] (device) = ||yref - out|| / max(||yref||, tol).  Synchronises (its core table is uploaded from the host). */
int ttn_cross_maxvol(int cplx, int64_t m, int64_t r, const double* A, double tol, int64_t maxiter, int64_t* piv, double* C, int64_t* dinfo,
                     int64_t* hinfo);
int ttn_cross_points(int cplx, int mode, int64_t N, int64_t site, int64_t n1, int64_t n2, int64_t rl, int64_t rr, const int64_t* L,
                     const int64_t* R, const int64_t* idx_in, int64_t P, const int64_t* doff, const double* dom, int64_t* idx_out, double* X);
int ttn_cross_eval(int cplx, int64_t N, int64_t P, const double* const* cores, const int64_t* dims, const int64_t* rks, const int64_t* idx,
                   const double* w, double* out, const double* yref, double tol, double* err);

/* ---- TT operator algebra (csrc/ttn_opalg_kernels.h), Float64.  A ttn_tto is immutable and its ranks are known on the host, so
 * every operation returns a NEW handle in *out (release it with ttn_tto_free); *out is written only on success.  Refused before
 * any launch: null pointers (TTN_ERR_ARG), an output core with 2^31 or more fibres r_{k-1} r_k (TTN_ERR_UNSUPPORTED: 32-bit element
 * indices), a result that does not fit in device memory (TTN_ERR_CAPACITY).  Asynchronous on the library stream unless stated.
 *   ttn_tto_mul      A * B (src/tt_operations.jl:162-172): ranks A.rks .* B.rks, A's bond index fastest; dims must agree (TTN_ERR_DIMS).
 *   ttn_tto_inner    the inner core product (:198-216): dims and ranks multiply, A major and B minor on every axis; d must agree.
 *   ttn_tto_add      A + B (:71-95), d >= 2 (d = 1: TTN_ERR_UNSUPPORTED, as ttn_add); ttn_tto_scale  a * A (:271-281: the first core
 *                    with ot == 0, else core 1; a == 0: zeros_tto with A's ranks, ot reset).  Both run the kernels of ttn_add /
 *                    ttn_scale on the operator seen as a vector (an operator core (n, n, r, r') is the vector core (n^2, r, r')).
 *   ttn_tto_kron     kron(A, B) (:427-433) and concatenate(A, B) (src/tt_tools.jl:723-735): needs A.rks[end] == B.rks[0] (TTN_ERR_DIMS).
 *   ttn_tt_outer     outer_product(x_b, y_b) (:297-304; real: no conjugate); ttn_tt_diag_tto  ttv_to_diag_tto(x_b) (:310-338).  Both
 *                    synchronise to read the current ranks of train b.
 *   ttn_tt_kron      z_t = kron(x_t, y_t) (:440-448) for every train t; z has d_x + d_y sites; the joint ranks must be 1.
 *   ttn_tto_to_tt    tto_to_ttv(A) (src/tt_tools.jl:296-304) into every train of y (dims n_k^2, capacity >= A's ranks).
 *   ttn_tto_from_tt  ttv_to_tto(x_b) (:323-333) with the current ranks (synchronises); a non-square dimension is TTN_ERR_DIMS.
 *   ttn_tto_compress tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps) as an operator: to_tt, ttn_compress, from_tt, all on the
 *                    device; a condition ttn_compress_status would report for the working train is this call's return value.
 *                    Synchronises.
 *   ttn_tto_ranks    d, dims (d), ranks (d + 1), ot (d) of a handle: any output may be null.  ttn_tto_set_ot: the gauge flags
 *                    (tto_ot) that ttn_tto_scale, ttn_tto_kron and ttn_tto_to_tt carry along; ttn_tto_create sets zeros.
 *   ttn_tto_download cores[k] receives n_k n_k rks[k] rks[k+1] doubles, column-major (synchronises). */
int ttn_tto_mul(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out);
int ttn_tto_inner(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out);
int ttn_tto_add(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out);
int ttn_tto_scale(double a, ttn_tto_t A, ttn_tto_t* out);
int ttn_tto_kron(ttn_tto_t A, ttn_tto_t B, ttn_tto_t* out);
int ttn_tt_outer(ttn_tt_t x, ttn_tt_t y, int64_t b, ttn_tto_t* out);
int ttn_tt_diag_tto(ttn_tt_t x, int64_t b, ttn_tto_t* out);
int ttn_tt_kron(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z);
int ttn_tto_to_tt(ttn_tto_t A, ttn_tt_t y);
int ttn_tto_from_tt(ttn_tt_t x, int64_t b, ttn_tto_t* out);
int ttn_tto_compress(ttn_tto_t A, int64_t max_bond, double truncerr, int64_t sweeps, ttn_tto_t* out);
int ttn_tto_ranks(ttn_tto_t A, int64_t* d, int64_t* dims, int64_t* rks, int64_t* ot);
int ttn_tto_set_ot(ttn_tto_t A, const int64_t* ot);
int ttn_tto_download(ttn_tto_t A, double* const* cores);

/* fused convenience for the benchmark op  tt_compress!(A*x, max_bond)  (src/solvers/euler.jl:55) */
int ttn_apply_compress(ttn_tto_t A, ttn_tt_t x, ttn_tt_t y, int64_t max_bond, double truncerr, int64_t sweeps);

/* out[b] = dot(a_b, b_b)      src/tt_operations.jl:239-250 ; out is HOST memory, length batch (synchronises) */
int ttn_dot(ttn_tt_t a, ttn_tt_t b, double* out);
/* HIP-event time of the KERNEL of the last ttn_dot / ttn_norm / ttn_orthogonalize / ttn_tto_mul call alone, or of the gather of the last
 * ttn_tto_decomp_dev (its three table launches and k_dense_gather, without the decomposition) (ttn_dot itself goes on to copy the
 * results to the host and synchronises, which an event pair around the call would include) — what bench.py --op reports.  Its
 * events are its own: such a call inside a ttn_timer_begin / ttn_timer_end region does not move the timer's start. */
int ttn_last_launch_ms(float* ms);
/* out[b] = norm(a_b) = sqrt(max(dot(a,a),0))   src/tt_operations.jl:465-470 */
int ttn_norm(ttn_tt_t a, double* out);

/* ---- core gradients (csrc/ttn_grad_kernels.h): the two reverse-mode rules of the reference's ChainRulesCore extension
 * (ext/TensorTrainNumericsChainRulesCoreExt) and the core-wise linear algebra of their tangents.  Float64 only.  A TANGENT (Abar, Bbar,
 * xbar, a gradient, a search direction) lives in an ordinary ttn_tt handle used as a bag of cores with the primal's current ranks per
 * train; its `ot` flags are 0 and it is never contracted as a train.
 *   ttn_dot_pullback    the rrule of dot(A, B) (ChainRulesCoreExt.jl:36-65): with the environments L_1 = [1], L_{k+1}[a,b] = sum A_k[z,al,a]
 *                       B_k[z,be,b] L_k[al,be] and G_{N+1} = [1], G_k[al,be] = sum A_k[z,al,a] B_k[z,be,b] G_{k+1}[a,b] (:8-34),
 *                       Abar_k[z,al,a] = Delta_b sum L_k[al,be] B_k[z,be,b] G_{k+1}[a,b] and Bbar_k with A and B exchanged.  delta: HOST,
 *                       `batch` doubles, NULL = 1.  abar / bbar may each be NULL, not both; abar receives a's current ranks (copied on
 *                       the device), bbar b's.  out: HOST or NULL; non-NULL: receives dot(a_b, b_b) = L_{N+1}[1,1] and the call
 *                       synchronises like ttn_dot; NULL (and delta NULL: a non-NULL delta is copied from caller memory first, which
 *                       waits for the stream) the call is asynchronous.  a and b may be the same handle; their ranks are independent.
 *                       Each environment is computed once per call (O(N) chain steps) and stays in library workspace:
 *                       2 (N + 1) W + 2 n_max rA_max rB_max doubles per train, W = max_m rA_m rB_m over the host-side rank bounds; a
 *                       workspace that cannot be allocated returns the allocator's error before any launch.
 *   ttn_apply_pullback  the rrule of H * psi with respect to psi (:67-88): xbar_k[j,vl,vr] = sum H_k[i,j,al,ar] ybar_k[i, al + R_{k-1} vl,
 *                       ar + R_k vr] (the operator index fastest in the merged rank, as ttn_apply writes it).  x is the primal: it gives
 *                       xbar its ranks, its cores are not read.  ybar must hold, per train, the ranks R .* (ranks of x).  Asynchronous.
 *   ttn_tt_cores_axpby  y_k <- alpha_b x_k + beta_b y_k on every core; alpha, beta: HOST, `batch` doubles each, NULL = 1 (a non-NULL one
 *                       is copied first, which waits for the stream; otherwise asynchronous).  x may be y.  Needs equal current ranks.
 *   ttn_tt_cores_dot    out[b] = sum_k <x_k, y_k>, the Frobenius pairing of two tangents (test_ad.jl: ladot); out: HOST; synchronises;
 *                       summed in a fixed order: a repeated call returns the same bits.
 * Before any launch: NULL pointer, bad handle, aliased output TTN_ERR_ARG; dims or batch differ TTN_ERR_DIMS; destination capacity below
 * the source's host-side rank bounds TTN_ERR_CAPACITY; a ComplexF64 handle or a train of 2^31 doubles or more TTN_ERR_UNSUPPORTED with a
 * message naming the call.  Ranks are device-resident, so the kernels check each train's own ranks themselves (ybar against R .* x; x
 * against y): a mismatch records a per-train code on the DESTINATION that ttn_compress_status reports as TTN_ERR_DIMS, that train's
 * destination cores are not written (ttn_tt_cores_dot: out[b] = NaN), every other train is computed.  Operands are only read. */
int ttn_dot_pullback(ttn_tt_t a, ttn_tt_t b, const double* delta, ttn_tt_t abar, ttn_tt_t bbar, double* out);
int ttn_apply_pullback(ttn_tto_t A, ttn_tt_t x, ttn_tt_t ybar, ttn_tt_t xbar);
int ttn_tt_cores_axpby(const double* alpha, ttn_tt_t x, const double* beta, ttn_tt_t y);
int ttn_tt_cores_dot(ttn_tt_t x, ttn_tt_t y, double* out);

/* z = hadamard(x, y)   src/tt_operations.jl:343-361 */
int ttn_hadamard(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z);
/* z = x + y            src/tt_operations.jl:10-35 (also the body of add!, :37-66) */
int ttn_add(ttn_tt_t x, ttn_tt_t y, ttn_tt_t z);
/* y = a * x            src/tt_operations.jl:256-266 (scales the first core with ot==0, else core 1;
 *                      a == 0 gives the all-zero train with ot reset to 0) */
int ttn_scale(double a, ttn_tt_t x, ttn_tt_t y);
/* y_b = a[b] * x_b with one factor per train (a is HOST memory, length batch): what `(1 / sqrt(dot(u, u))) * u` needs on a
 * batch (src/solvers/euler.jl:83-85, :205-207) */
int ttn_scale_batch(const double* a, ttn_tt_t x, ttn_tt_t y);
/* y = orthogonalize(x; i=center)   src/tt_tools.jl:511-543 ; center is 1-based.  QTT trains of rank <= 64 take three kernels
 * (csrc/ttn_ortho_ramp.h: one wave per train over the rank-ramp sites; csrc/ttn_ortho512.h: Cholesky-QR steps with a measured
 * orthogonality check over the tall sites and the centre core; the 1024-thread k_orthogonalize for the left sweep and for trains the
 * other two refuse) and the call reads one word back between them (it synchronises the library stream once); every other train
 * class is one asynchronous launch.  TTN_ORTHO512 = 0 / 1 forbids / forces the multi-kernel form; TTN_ORTHO_CHOLQR = 1 switches its
 * Cholesky-QR steps off (A/B runs, parity tests of the general route). */
int ttn_orthogonalize(ttn_tt_t x, int64_t center, ttn_tt_t y);

/* ---- parity instrumentation: singular values seen by the last ttn_compress / ttn_bond_truncate --
 * After ttn_sv_capture(h, 1), each bond step stores ALL singular values of its merged matrix (sorted,
 * descending, before truncation).  `step` counts bond steps of the last call from 0
 * (L->R k=1..N-1, then R->L k=N-1..1, per sweep).  Returns the count in *n (<= cap). */
int ttn_sv_capture(ttn_tt_t h, int enable);
int ttn_sv_get(ttn_tt_t h, int64_t b, int64_t step, double* out, int64_t cap, int64_t* n);

/* ---- timing on the library stream (HIP events) ------------------------------------------------- */
/* begin / end bracket everything enqueued between them (events of their own, see ttn_last_launch_ms) */
int ttn_timer_begin(void);
int ttn_timer_end(float* ms);   /* synchronises */
/* event slots (0..4095) recorded on the library stream without synchronising; elapsed() synchronises */
int ttn_event_record(int64_t slot);
int ttn_event_elapsed(int64_t slot_a, int64_t slot_b, float* ms);

/* kernel unit-test hook: C (m x n row-major, host, in/out) = alpha*op(A)*op(B) + beta*C computed by the device-side
 * workgroup GEMM (fp64 MFMA) every dense kernel is built on; ta/tb: operand stored transposed */
int ttn_selftest_gemm(int64_t m, int64_t n, int64_t k, const double* A, const double* B, double* C, double alpha, double beta,
                      int ta, int tb);

/* kernel unit-test hook of the two-team Gram product of a bond step: G_i (p_i x p_i row-major, host, in/out) = alpha_i A_i A_i^T for
 * i = 1, 2 in ONE single-workgroup launch; A_i stored p_i x q_i row-major, or q_i x p_i if ta_i.  pair = 1: one paired call;
 * pair = 0: two single calls in the same launch (the reference the paired call must match bit for bit) */
int ttn_selftest_syrk2(int64_t p1, int64_t q1, const double* A1, double* G1, double alpha1, int ta1,
                       int64_t p2, int64_t q2, const double* A2, double* G2, double alpha2, int ta2, int pair);

/* kernel unit-test hook of the two-team register-A product of a bond step: C_i (m_i x n_i, host, in/out) = alpha_i A_i B_i for i = 1, 2 in
 * ONE single-workgroup launch; row-major operands, f_i & 1 / 2 / 4: A_i / B_i / C_i stored transposed.  pair = 1: one paired call;
 * pair = 0: two single calls in the same launch (the reference the paired call must match bit for bit) */
int ttn_selftest_gemm_ra2(int64_t m1, int64_t n1, int64_t k1, const double* A1, const double* B1, double* C1, double alpha1, int f1,
                          int64_t m2, int64_t n2, int64_t k2, const double* A2, const double* B2, double* C2, double alpha2, int f2, int pair);

/* kernel unit-test hook of the dense local solve of als / mals / dmrg_linsolve: K x = rhs by the blocked LU with partial pivoting (first
 * maximal |entry| of the column, as LAPACK's idamax).  K host, N x N column-major; rhs, x_out N doubles; piv_out[j] = the 0-based row
 * exchanged with row j at step j (LAPACK's ipiv - 1; -1 for a column the elimination did not reach).  form 0: wg_lu_solve, one
 * workgroup, N <= 2048; form 1: the grid-form stages of csrc/ttn_als_grid.h, N <= 8192.  Returns 0, or 1 if a pivot column is exactly
 * zero (x_out then holds the partly eliminated right-hand side: finite, not a solution), or a TTN_ERR_* code. */
int ttn_selftest_lu_solve(int64_t N, const double* K, const double* rhs, double* x_out, int64_t* piv_out, int form);
/* kernel unit-test hook of the matrix-free two-site operator (wg_two_site_apply, shared by the CG local solver and the two-site
 * eigensolvers): out = 1/2 (K + K^T) v with K[(ab,cd),(ef,gh)] = sum_z G[ab,ef,z] H[z,cd,gh].  Host arrays: G (na, na, Rz)
 * column-major, H (Rz, nb, nb) with z fastest, v and out na x nb column-major.  1 <= na, nb <= 256, 1 <= Rz <= 64. */
int ttn_selftest_two_site_apply(int64_t na, int64_t nb, int64_t Rz, const double* G, const double* H, const double* v, double* out);

/* self-test of the symmetric eigensolver used by the Gram routes (csrc/ttn_eig_kernels.h): G host, n x n (n = 64 or 128),
 * column-major, symmetric positive definite; sig[nev] = sqrt of the nev largest eigenvalues (descending), X[128*r] = sig_j * u_j (r <= 64);
 * ticks_rc[0] = device clock ticks of the whole routine, [1] = its return code; ticks_rc has 2 entries. */
int ttn_selftest_eig128(const double* G, int64_t n, int64_t r, int64_t nev, double* sig, double* X, int64_t* ticks_rc);
/* self-test of the dense symmetric eigensolver of the two-site eigensolvers (wg_sym_eig_smallest, csrc/ttn_eigsolve_kernels.h): A host,
 * N x N, column-major, symmetric (both triangles); lam[k] = the k smallest eigenvalues ascending, Y[N*k] = their orthonormal vectors as
 * columns (no sign normalisation).  1 <= N <= 2048, 1 <= k <= min(N, 16); TTN_ERR_ARG otherwise, before anything is launched. */
int ttn_selftest_sym_eig(int64_t N, int64_t k, const double* A, double* lam, double* Y);
/* poison mode, a test switch (host side only, off by default).  While on: the per-call workspace is filled with the 8-byte
 * `pattern` at every acquisition, before the entry point's first launch or copy into it; a new ttn_tt arena holds the pattern outside the
 * live block of its rank-1 zero trains (the first el * n_k doubles of every slot stay zero); a new ttn_tto arena holds it wherever no core
 * is uploaded; the self-test hooks above fill their workspace and output allocations with it instead of clearing them or leaving them
 * raw.  No kernel differs.  on = 0 ends the mode (pattern ignored), and so does ttn_finalize.  Always TTN_OK. */
int ttn_selftest_poison(int on, uint64_t pattern);
/* probe: takes nbytes (>= 8) of the per-call workspace as an entry point does and returns the first 8 bytes and the last whole 8-byte
 * word of the whole buffer (in poison mode: the pattern, twice) */
int ttn_selftest_workspace_peek(int64_t nbytes, uint64_t* out_first8, uint64_t* out_last8);
/* probe: a raw read of n doubles of train b's arena from double `offset` on (slot k starts at the sum of the earlier slots'
 * el * n_j * cap_j * cap_{j+1}, each rounded up to even), live block and slack alike; offset + n within the train's arena */
int ttn_selftest_tt_peek(ttn_tt_t h, int64_t b, int64_t offset, int64_t n, double* out);
/* diagnostics of the last ttn_orthogonalize when it took the multi-launch form (csrc/ttn_ortho_ramp.h, ttn_ortho512.h): the four state
 * words of train b = {next site of the right-to-left sweep, buffer of the last right factor, buffer of the last left factor,
 * 1 if k_ortho512 finished the train (0: the 1024-thread kernel took it over from `next site`)}.  Read from the library's workspace:
 * meaningful until the next call that uses it; TTN_ERR_ARG if b is outside the batch of that orthogonalize. */
int ttn_debug_ortho_state(int64_t b, int64_t* out4);

/* ---- stateless host-pointer entry points: the literal drop-ins for one train --------------------
 * Each uploads, runs the handle op above, and downloads.  Output cores are caller-allocated:
 *   apply     : Y_cores[k] sized n_k*(A_rks[k]*X_rks[k])*(A_rks[k+1]*X_rks[k+1])   (as zeros_tt would)
 *   hadamard  : Z_cores[k] sized n_k*(rx*ry)_k*(rx*ry)_{k+1}
 *   add       : Z_cores[k] sized with ranks rx+ry (ends forced to 1)
 *   compress  : in/out cores sized n_k*need[k]*need[k+1] with need from ttn_compress_rank_bound (= the input
 *               ranks unless a rank-deficient bond can grow); on entry they hold the input cores compactly,
 *               on exit the new cores compactly; `rks` is updated in place
 *   orthogonalize: Y_cores sized for X_rks (output ranks never exceed the input's) ; Y_rks / Y_ot are outputs
 */
int ttn_apply_f64(int64_t d, const int64_t* dims,
                  const double* const* A_cores, const int64_t* A_rks,
                  const double* const* X_cores, const int64_t* X_rks,
                  double* const* Y_cores);
int ttn_dot_f64(int64_t d, const int64_t* dims,
                const double* const* A_cores, const int64_t* A_rks,
                const double* const* B_cores, const int64_t* B_rks, double* out);
int ttn_hadamard_f64(int64_t d, const int64_t* dims,
                     const double* const* X_cores, const int64_t* X_rks,
                     const double* const* Y_cores, const int64_t* Y_rks,
                     double* const* Z_cores);
int ttn_add_f64(int64_t d, const int64_t* dims,
                const double* const* X_cores, const int64_t* X_rks,
                const double* const* Y_cores, const int64_t* Y_rks,
                double* const* Z_cores);
int ttn_scale_f64(int64_t d, const int64_t* dims, double a,
                  const double* const* X_cores, const int64_t* X_rks, const int64_t* X_ot,
                  double* const* Y_cores, int64_t* Y_ot);
int ttn_orthogonalize_f64(int64_t d, const int64_t* dims,
                          const double* const* X_cores, const int64_t* X_rks, int64_t center,
                          double* const* Y_cores, int64_t* Y_rks, int64_t* Y_ot);
int ttn_compress_f64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks,
                     int64_t max_bond, double truncerr, int64_t sweeps);
int ttn_bond_truncate_f64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks,
                          int64_t k, int64_t max_bond, double truncerr);
/* op = x -> tt_compress!(A * x, max_bond) (src/solvers/euler.jl:55, the operator krylov_linsolve / the time steppers iterate) as ONE
 * stateless call: A * x is never materialised, neither in HBM nor over PCIe (fused apply).  Y_cores[k] sized n_k * cap_k * cap_{k+1}
 * with cap from ttn_apply_compress_rank_bound (the final ranks a sweep can leave: min(A_rks .* X_rks, max_bond, what the dimensions
 * allow)); Y_rks (d + 1) receives the ranks, the cores come back compactly with those ranks. */
int ttn_apply_compress_rank_bound(int64_t d, const int64_t* dims, const int64_t* A_rks, const int64_t* X_rks, int64_t max_bond, int64_t sweeps,
                                  int64_t* cap);
int ttn_apply_compress_f64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks,
                           const double* const* X_cores, const int64_t* X_rks, double* const* Y_cores, int64_t* Y_rks,
                           int64_t max_bond, double truncerr, int64_t sweeps);

/* ---- ComplexF64 trains and operators (csrc/ttn_cplx_kernels.h) ------------------------------------------------
 * The element type of a handle is fixed at creation: ttn_tt_create / ttn_tto_create make Float64 handles, the two creators below
 * ComplexF64 ones.  A complex core is the reference's Array{ComplexF64,3} as it lies: column-major (n, r_l, r_r) (operator:
 * (n, n, R_l, R_r)), interleaved (re, im); every `double*` that points at cores of a complex handle points at such pairs, so a core
 * of n r_l r_r numbers is 2 n r_l r_r doubles.  ttn_tt_upload / download / ranks / max_ranks / replicate / copy (same type on both
 * sides) / batch / free, ttn_tto_free / ranks / set_ot / download, ttn_compress_status and ttn_status_all work on either kind.
 * On ComplexF64 handles:
 *   ttn_apply           complex operator x complex train, REAL operator x complex train, complex operator x REAL train; y must be a
 *                       complex handle (k_zapply).  A complex y with a real operator and a real train is refused.
 *   ttn_add             all three complex (k_add on the (2n, r, r') real view of the cores: + only copies)
 *   ttn_hadamard        all three complex, no conjugation (tt_operations.jl:343-361)
 *   ttn_scale           real factor; ttn_scale_c64 a complex one (re, im); ttn_scale_batch_c64 one complex factor per train
 *                       (a: HOST, `batch` interleaved pairs).  The reference's rule: the first core with ot == 0, else core 1; a == 0
 *                       gives the zero train with ot reset.
 *   ttn_dot             both complex; the FIRST argument is conjugated (tt_operations.jl:243-248); `out` receives `batch` interleaved
 *                       (re, im) pairs, i.e. 2 * batch doubles.  ttn_norm: `batch` doubles, sqrt(max(real(dot(a, a)), 0)).
 *   ttn_compress, ttn_bond_truncate, ttn_sweep   the contract of the Float64 calls (one workgroup per train, device-resident ranks, the
 *                       same rank rule, sqrt(s) on both sides, no gauge step): Householder QR of the long side, then one-sided
 *                       complex Jacobi on the square factor of the short side.  Limits: merged matrices with short side <= 512 and
 *                       long side <= 8192 complex numbers (TTN_ERR_UNSUPPORTED before any launch).
 *   ttn_apply_compress  ttn_apply, then ttn_compress (no fused complex merge); every check runs before y is touched.
 * Refused with TTN_ERR_UNSUPPORTED before any launch, with a message that names the call: a call above whose vector operands differ
 * in element type, and a ComplexF64 handle given to any Float64-only entry point: the linear solvers and eigensolvers,
 * ttn_orthogonalize, ttn_hadamard_ttm, ttn_swap_sites, ttn_ttv_decomp, ttn_scale_batch, the operator algebra (ttn_tto_mul / inner /
 * add / scale / kron / compress / to_tt / from_tt, ttn_tt_outer / diag_tto / kron), ttn_apply_begin / _sweep, ttn_tt_core_extent /
 * _export / _import, ttn_sv_capture, ttn_tt_to_dense, ttn_tto_to_dense, ttn_ttv_decomp_dev, ttn_tt_split_sites, ttn_tt_merge_sites. */
int ttn_tt_create_c64(int64_t d, const int64_t* dims, const int64_t* cap_rks, int64_t batch, ttn_tt_t* out);
int ttn_tto_create_c64(int64_t d, const int64_t* dims, const int64_t* rks, const double* const* cores, ttn_tto_t* out);
int ttn_tt_dtype(ttn_tt_t h, int* cplx);      /* *cplx = 0 Float64, 1 ComplexF64 */
int ttn_tto_dtype(ttn_tto_t h, int* cplx);
int ttn_scale_c64(double re, double im, ttn_tt_t x, ttn_tt_t y);
int ttn_scale_batch_c64(const double* a, ttn_tt_t x, ttn_tt_t y);
/* Stateless ComplexF64 drop-ins for one train: the argument lists of the _f64 calls, every core buffer interleaved.  apply and
 * apply_compress take the two mixed forms too: a_cplx / x_cplx say whether the operator / the train is complex (at least one must
 * be); Y is always complex.  ttn_dot_c64: out[0], out[1] = re, im.  ttn_scale_host_c64: the factor is (re, im). */
int ttn_apply_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                  const int64_t* X_rks, double* const* Y_cores, int a_cplx, int x_cplx);
int ttn_dot_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* B_cores,
                const int64_t* B_rks, double* out);
int ttn_hadamard_c64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, const double* const* Y_cores,
                     const int64_t* Y_rks, double* const* Z_cores);
int ttn_add_c64(int64_t d, const int64_t* dims, const double* const* X_cores, const int64_t* X_rks, const double* const* Y_cores,
                const int64_t* Y_rks, double* const* Z_cores);
int ttn_scale_host_c64(int64_t d, const int64_t* dims, double re, double im, const double* const* X_cores, const int64_t* X_rks,
                       const int64_t* X_ot, double* const* Y_cores, int64_t* Y_ot);
int ttn_compress_c64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t max_bond, double truncerr, int64_t sweeps);
int ttn_bond_truncate_c64(int64_t d, const int64_t* dims, double* const* cores, int64_t* rks, int64_t k, int64_t max_bond, double truncerr);
int ttn_apply_compress_c64(int64_t d, const int64_t* dims, const double* const* A_cores, const int64_t* A_rks, const double* const* X_cores,
                           const int64_t* X_rks, double* const* Y_cores, int64_t* Y_rks, int64_t max_bond, double truncerr, int64_t sweeps,
                           int a_cplx, int x_cplx);

/* r_and_d_to_rks(rks, dims; rmax)   src/tt_tools.jl:407-425 (host-side integer helper, bit-exact) */
int ttn_r_and_d_to_rks(int64_t d, const int64_t* dims, int64_t n_rks, const int64_t* rks, int64_t rmax, int64_t* out);

/* ---- rectangular operators: grid transfer (csrc/ttn_rect_kernels.h) ----------------------------------------------
 * The reference's second method of `*` (src/tt_operations.jl:116-148): an operator of M = N + 1 sites with cores
 * (n_out, n_in, R_l, R_r), exactly one of them with n_in == 1, applied to trains of N sites: qtto_constant_prolongation and
 * qtto_linear_prolongation (src/tt_operators.jl:441-504).  Such an operator lives in a handle type of its own, ttn_rtto_t, so that no
 * entry point above can be handed one; the type and its five entry points (ttn_rtto_create / free / ranks, ttn_apply_rect,
 * ttn_apply_rect_f64) are declared in ttn_rect.h, which this header includes. */
#include "ttn_rect.h"

/* ---- the dense bridge for operators (csrc/ttn_grid_kernels.h) -----------------------------------------------------
 * tto_to_tensor / qtto_to_matrix and tto_decomp on the device: ttn_tto_to_dense writes an operator into a dense array addressed by
 * two stride tables, ttn_tto_decomp_dev turns such an array into an operator (gather kernel + the hierarchical SVD of
 * ttn_ttv_decomp_dev).  Both are declared in ttn_dense.h, which this header includes. */
#include "ttn_dense.h"

/* ---- time steps (csrc/ttn_step_kernels.h) --------------------------------------------------------------------------
 * What the steppers of src/solvers/euler.jl do around their linear solve: ttn_apply_axpby, z = alpha x + beta (A y) in one streaming
 * launch, and ttn_tt_increase_ranks, the public increase_ranks.  Both are declared in ttn_step.h, which this header includes. */
#include "ttn_step.h"

/* ---- MaxVol cross for a batch of functions (csrc/ttn_cross_batch_kernels.h) ----------------------------------------
 * The per-site work of tt_cross(f, domain, ::MaxVol) for many functions in one launch: ttn_cross_batch_points (fibre index matrices and
 * coordinates from per-function sets), ttn_cross_batch_site (scale, QR, maxvol, core and next index set, one workgroup per function)
 * and ttn_cross_batch_eval (validation error or weight contraction per function).  Declared in ttn_cross_batch.h, which this header
 * includes. */
#include "ttn_cross_batch.h"

/* ---- expectation values (csrc/ttn_expect_kernels.h) ----------------------------------------------------------------
 * <x, A y> per train without forming A y: ttn_sandwich (result on the host, synchronises as ttn_dot) and ttn_sandwich_dev (result in
 * device memory, asynchronous).  Declared in ttn_expect.h, which this header includes. */
#include "ttn_expect.h"

/* ---- the gradient of an expectation value (csrc/ttn_expect_grad_kernels.h) ------------------------------------------
 * ttn_sandwich_pullback: the tangents of <x, A y> with respect to the cores of x and y on the three-layer environments, A y never
 * formed.  Declared in ttn_expect_grad.h, which this header includes. */
#include "ttn_expect_grad.h"

/* ---- operator batches (csrc/ttn_opbatch_kernels.h) ------------------------------------------------------------------
 * B operators of equal dims and ranks in one ttn_tto handle, operator b for train b: ttn_tto_create_batch, ttn_tto_from_tt_batch,
 * ttn_tto_batch, ttn_tto_select, ttn_tto_download_b, and the list of the entry points above that take such a handle (every other one
 * refuses it).  Declared in ttn_opbatch.h, which this header includes. */
#include "ttn_opbatch.h"

/* ---- site-resolved measurements (csrc/ttn_measure_kernels.h) --------------------------------------------------------
 * The profile <x| O_k |x> / <x, x> of every site and the two-point functions <x| P_i Q_j |x> / <x, x> of ALL pairs, per train, from one
 * pair of environment chains: ttn_site_expect, ttn_correlation and their _dev forms.  Declared in ttn_measure.h, which this header
 * includes. */
#include "ttn_measure.h"

/* ---- sampling (csrc/ttn_sample_kernels.h) ---------------------------------------------------------------------------
 * Configurations drawn from p(z) = x(z)^2 / <x, x> (Born) or p(z) = x(z) / sum x (density) with their log-probabilities, per train, by
 * the conditional sweep over the sites: ttn_tt_sample, ttn_tt_sample_dev, ttn_tt_sample_last_ms.  Declared in ttn_sample.h, which this
 * header includes. */
#include "ttn_sample.h"

/* ---- excited states (csrc/ttn_eig_ortho_kernels.h) ------------------------------------------------------------------
 * The two-site eigensolvers with a penalty against given trains, the local problem K + sum_j w_j p_j p_j^T: ttn_dmrg_eigsolve_ortho,
 * ttn_mals_eigsolve_ortho.  Declared in ttn_eig_ortho.h, which this header includes. */
#include "ttn_eig_ortho.h"

/* ---- <x| A |y> on ComplexF64 operands (csrc/ttn_braket_kernels.h) ---------------------------------------------------
 * sum_{i, j} conj(x_i) A_ij y_j per train without forming A y, for complex or real trains and a complex or real operator: ttn_braket
 * (result on the host, synchronises as ttn_dot) and ttn_braket_dev (device memory, asynchronous).  Declared in ttn_braket.h, which
 * this header includes. */
#include "ttn_braket.h"

/* ---- the fixed-rank TT manifold (csrc/ttn_tangent_kernels.h) ----------------------------------------------------------
 * The orthogonal projection of a train onto the tangent space at a point given by its two gauges, and the train alpha x + beta xi of a
 * tangent at twice the ranks: ttn_tangent_project, ttn_tangent_to_tt.  Declared in ttn_tangent.h, which this header includes. */
#include "ttn_tangent.h"

/* ---- partial contraction of a train (csrc/ttn_contract_kernels.h) ------------------------------------------------------
 * A subset of the sites contracted against weight vectors, the result a train on the remaining sites — marginals, slices and moments
 * of function-valued trains without a dense array: ttn_tt_contract_sites.  Declared in ttn_contract.h, which this header includes. */
#include "ttn_contract.h"

/* ---- site-resolved measurements on ComplexF64 trains (csrc/ttn_zmeasure_kernels.h) -------------------------------------
 * The complex profile <x| O_k |x> / <x|x> of every site and the two-point functions <x| P_i Q_j |x> / <x|x> of ALL pairs, per train, the
 * bra conjugated and the tables complex (a lone sigma_y included): ttn_zsite_expect, ttn_zcorrelation and their _dev forms.  Declared
 * in ttn_zmeasure.h, which this header includes. */
#include "ttn_zmeasure.h"

#ifdef __cplusplus
}
#endif
#endif /* TTN_H */
