"""Power-of-two scaling of trains and operators, in plain NumPy (no device code): the helpers of tests/test_cpu_scale.py and
tests/test_gpu_scale.py.

SVD truncation with a relative rule, QR and the inner product are homogeneous: op(c x) = c op(x) with the same ranks.  LAPACK gets
that by scaling internally; the device kernels get it by hand ("in units of s0 = max|M|"), and a product like 1 / (s0 s0) leaves the
double range long before the data does.  The tests feed the kernels x scaled by 2^e and compare with the result for the UNSCALED x:

  balanced(x)            every core divided by a power of two so that each left partial product of the train has a norm in
                         [2^-1/2, 2^1/2]: after it the exponent a test states is the exponent a kernel sees (a d = 30, rank-64
                         random train otherwise brings 2^103 of its own).
  scaled(x, place, e)    2^e put into the first, last or middle core, or 2^e into core m and 2^-e into core m + 1 ("graded": the
                         tensor is unchanged).  numpy.ldexp only: every scaling is exact.
  unscaled(y, e)         y times 2^-e, exactly, split over two cores so that no intermediate leaves the range.
  sv_ratios(s)           sigma_i / sigma_1: what is compared of the captured singular values (the sqrt(S) split of a bond step hands
                         2^(e/2), 2^(e/4), ... down the sweep, so later steps' absolute values are no power-of-two multiples).

The reference for a scaled input is ALWAYS the oracle's result on the unscaled input, never the oracle on the scaled input: with
truncerr > 0 the oracle's rank rule squares the singular values (oracle/tt_oracle.py, svdtrunc) and is itself not covariant outside
about 2^+-500 (tests/test_cpu_scale.py pins the two observations)."""
import numpy as np

from oracle import tt_oracle as O

PLACEMENTS = ("first", "last", "middle", "graded")
MODERATE = (200, -200)          # values, squares and fourth powers stay normal
FAR = (800, -800)               # values stay normal with 2^200 of headroom; squares do not


def _field(x):
    return "ttv_vec" if hasattr(x, "ttv_vec") else "tto_vec"


def cores_of(x):
    return list(getattr(x, _field(x)))


def with_cores(x, cores):
    """A new train / operator of x's type (oracle or product) with the given cores; x is not touched."""
    if hasattr(x, "ttv_vec"):
        return type(x)(x.N, list(cores), tuple(x.ttv_dims), list(x.ttv_rks), list(x.ttv_ot))
    return type(x)(x.N, list(cores), tuple(x.tto_dims), list(x.tto_rks), list(x.tto_ot))


def ldexp(a, e):
    """a * 2^e, exact (as long as nothing over- or underflows); real or complex arrays, layout kept."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        out = np.empty_like(a)
        out.real = np.ldexp(a.real, e)
        out.imag = np.ldexp(a.imag, e)
        return out
    return np.ldexp(a, e)


def _as3(c):
    """(n, rl, rr) view of a train core, (n*m, rl, rr) of an operator core."""
    return c.reshape((-1,) + c.shape[-2:])


def partial_norms(x, dtype=np.longdouble):
    """Frobenius norms of the left partial products G_1 ... G_k, k = 1..d, accumulated in `dtype` (real trains)."""
    out = []
    M = np.ones((1, 1), dtype=dtype)
    for c in cores_of(x):
        c3 = _as3(np.asarray(c)).astype(dtype)
        M = sum(c3[z].T @ (M @ c3[z]) for z in range(c3.shape[0]))
        out.append(np.sqrt(np.trace(M)))
    return out


def balanced(x):
    """Every core divided by a power of two, chosen site by site so that the norm of the left partial product G_1 ... G_k lands in
    [2^-1/2, 2^1/2] (for a random core the divisor is about 2^round(log2(sqrt(n r))); the residual of each rounding is carried into
    the next site instead of piling up over d sites)."""
    cores = []
    M = np.ones((1, 1))
    for c in cores_of(x):
        c3 = _as3(np.asarray(c))
        M = sum(np.conj(c3[z]).T @ (M @ c3[z]) for z in range(c3.shape[0]))
        t = float(np.sqrt(np.real(np.trace(M))))
        e = int(np.rint(np.log2(t))) if t > 0 and np.isfinite(t) else 0
        cores.append(ldexp(c, -e))
        M = ldexp(M, -2 * e)
    return with_cores(x, cores)


def middle(d):
    """ceil(d / 2), 1-based"""
    return (d + 1) // 2


def scaled(x, placement, e):
    cores = [np.array(c, order="K") for c in cores_of(x)]
    d = len(cores)
    m = middle(d)
    if placement == "first":
        cores[0] = ldexp(cores[0], e)
    elif placement == "last":
        cores[d - 1] = ldexp(cores[d - 1], e)
    elif placement == "middle":
        cores[m - 1] = ldexp(cores[m - 1], e)
    elif placement == "graded":
        assert d >= 2 and m < d
        cores[m - 1] = ldexp(cores[m - 1], e)
        cores[m] = ldexp(cores[m], -e)
    else:
        raise ValueError(placement)
    return with_cores(x, cores)


def total_exponent(placement, e):
    """the power of two the TENSOR is multiplied by"""
    return 0 if placement == "graded" else e


def _core_exponent(c):
    a = float(np.max(np.abs(c))) if c.size else 0.0
    return int(np.frexp(a)[1]) if a > 0 and np.isfinite(a) else 0


def unscaled(y, e):
    """y * 2^-e, split in two halves; each half goes to the core that is then the largest (e > 0) or the smallest (e < 0), so a core
    never leaves the range on the way."""
    cores = [np.array(c, order="K") for c in cores_of(y)]
    for part in (e // 2, e - e // 2):
        if part == 0:
            continue
        ex = [_core_exponent(c) for c in cores]
        k = int(np.argmax(ex)) if part > 0 else int(np.argmin(ex))
        cores[k] = ldexp(cores[k], -part)
    return with_cores(y, cores)


def sv_ratios(s):
    s = np.asarray(s, dtype=np.float64)
    return s / s[0]


def all_finite(x):
    return all(bool(np.all(np.isfinite(np.asarray(c)))) for c in cores_of(x))


# ----------------------------------------------------------------------------------------------------------------------------
# The rounding cases: the smallest shapes at which each route of k_compress is known to be reached (tests/test_gpu_parity.py).
# name -> (builder, max_bonds).  A builder returns (A or None, x) as ORACLE objects, x balanced; the train that is rounded is
# A * x (fused: apply_compress(A, x)) or x itself.
# ----------------------------------------------------------------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(31)
    return None, balanced(O.rand_tt((3, 2, 5, 2, 3, 4), [1, 3, 5, 7, 6, 3, 1], rng))


def _delta_x(d, r, seed):
    def build():
        rng = np.random.default_rng(seed)
        return O.Delta(d), balanced(O.rand_tt((2,) * d, r, rng))
    return build


def _rand_op_x(d, r, seed):
    def build():
        rng = np.random.default_rng(seed)
        A = O.rand_tto((2,) * d, 3, rng)
        return balanced(A), balanced(O.rand_tt((2,) * d, r, rng))
    return build


# Singular values: sigma_i / sigma_1 of EVERY bond step is compared, with ONE static exception.  eig_r64 at max_bond 64 (d = 12, Delta
# times a rank-64 train, nominal ranks 192): the bonds right of the middle are rank deficient (3 r_k exceeds what the sites right of
# them can carry), the reference keeps min(length(s), max_bond) directions there, noise included (48 at a bond of true rank 16), and
# the sqrt(S) gauge hands those noise directions (sqrt(1e-17) = 3e-9 in each factor) to the steps of the returning sweep.  Their
# singular values then depend on rounding noise at the 1e-12 sigma_1 level: the oracle against ITSELF under scaling differs by up to
# 3e-12 there (tests/test_cpu_scale.py measures and pins it), while the tensor agrees to 1e-14.  For that one case the comparison
# covers the steps of the first left-to-right sweep, which are functions of the input alone.  With max_bond 50 or 20 the noise
# directions are cut and every step is compared.  Nothing is decided at run time.
SV_FIRST_SWEEP_ONLY = {("eig_r64", 64)}


def sv_steps_compared(name, max_bond, d, nsteps):
    return d - 1 if (name, max_bond) in SV_FIRST_SWEEP_ONLY else nsteps


def sv_atol(name):
    """the floors of tests/test_gpu_parity.py, in units of sigma_1: 1e-13, and 1e-12 where ranks above 64 are kept (256-row merged
    matrices, test_compress_ranks_up_to_128_blocked_jacobi)"""
    return 1e-12 if name == "short_side_200" else 1e-13

COMPRESS_CASES = {
    "small_step": (_small, (4,)),                                   # general dims, odd sizes
    "lds_routes_r24": (_delta_x(14, 24, 3), (24,)),                 # in-LDS routes G / F / H
    "eig_r64": (_delta_x(12, 64, 0), (64, 50, 20)),                 # 128 x 384 Gram + wg_eig128, route F on wg_eig64, CholeskyQR2 ramp
    "eig_r32": (_delta_x(12, 32, 6), (32,)),                        # 64 x 192 Gram steps on wg_eig64
    "pad96_r48": (_rand_op_x(14, 48, 4), (64,)),                    # the zero-padded 96-row step and its polish
    "short_side_200": (_delta_x(14, 70, 77), (100,)),               # merged short side 200 > 128: global-memory Jacobi + Householder
}


def compress_input(name):
    """(A, x, y) of a case: y = A x as an oracle train (x itself when the case has no operator)."""
    A, x = COMPRESS_CASES[name][0]()
    return A, x, (O.apply(A, x) if A is not None else x)


def scale_input(A, x, placement, e):
    """The scaling goes into the TRAIN x (the operator stays as it is): A (c x) = c (A x) core by core, exactly."""
    return scaled(x, placement, e)


ORTHO_CASES = ((9, 5, 2), (12, 20, 5), (16, 37, 1), (30, 64, 1), (30, 64, 30))      # (d, r, centre)


def ortho_input(d, r, center):
    rng = np.random.default_rng(500 + d + r + center)
    return balanced(O.rand_tt((2,) * d, r, rng))


DOT_CASES = ((12, 37, 64), (9, 65, 99))          # LDS path, generic path


def dot_input(d, ra, rb):
    rng = np.random.default_rng(d + ra)
    return balanced(O.rand_tt((2,) * d, ra, rng)), balanced(O.rand_tt((2,) * d, rb, rng))
