"""Inputs and CPU-side instruments of the linear-solver tests (test_gpu_als / _mals / _dmrg / _lu): operators whose local systems
make the pivoted LU exchange rows beyond its first panel, a non-symmetric operator with a positive-definite symmetric part for the
CG path, a spy that records what the oracle's local solves would make a partially pivoted LU do, and a longdouble elimination that
arbitrates pivot choices.  NumPy / SciPy only: every precondition a GPU test relies on is asserted with these on the CPU first."""
import contextlib

import numpy as np
import scipy.linalg as sla

from oracle import tt_oracle as O

LU_NB = 32          # panel width of wg_lu_solve / k_lu_panel (csrc/ttn_als_kernels.h)


def bitflip_tto(d):
    """X = [[0, 1], [1, 0]] on every site (rank 1): the permutation i -> 2^d - 1 - i."""
    X = np.array([[0.0, 1.0], [1.0, 0.0]]).reshape(2, 2, 1, 1)
    return O.TToperator(d, [X.copy() for _ in range(d)], (2,) * d, [1] * (d + 1), [0] * d)


def A_piv(d):
    """2 X + toeplitz(0.5, -0.7, 0.2): the dominant entries sit on the ANTI-diagonal, so Gaussian elimination has to exchange rows
    all the way down; non-symmetric, cond 3.4 at d = 8."""
    return O.tto_add(O.tto_scale(2.0, bitflip_tto(d)), O.toeplitz_to_qtto(0.5, -0.7, 0.2, d))


def A_cd(d):
    """Convection-diffusion stencil toeplitz(2.5, -1.6, -0.4): relative asymmetry 0.56, symmetric part positive definite (smallest
    eigenvalue 0.50), cond 8.9 at d = 6."""
    return O.toeplitz_to_qtto(2.5, -1.6, -0.4, d)


def id_general(dims):
    cores = [np.eye(n).reshape(n, n, 1, 1) for n in dims]
    return O.TToperator(len(dims), cores, tuple(dims), [1] * (len(dims) + 1), [0] * len(dims))


def mixed_dims_operator(dims, rng):
    """4 I + R, R = rand_tto(dims, 2) scaled to spectral norm 2: non-symmetric, symmetric part >= 2 I (CG applies), cond <= 3 —
    pinned by tests/test_cpu_linsolve_inputs.py."""
    R = O.rand_tto(dims, 2, rng)
    return O.tto_add(O.tto_scale(2.0 / np.linalg.norm(tto_to_matrix(R), 2), R), O.tto_scale(4.0, id_general(dims)))


def tto_to_matrix(A):
    """Dense matrix of a TT operator with any physical dimensions, site 1 most significant (qtto_to_matrix's order)."""
    M = np.ones((1, 1, 1))                                       # (rows, cols, bond)
    for c in A.tto_vec:
        M = np.einsum("pqa,ijab->piqjb", M, c).reshape(M.shape[0] * c.shape[0], M.shape[1] * c.shape[1], c.shape[3])
    return M[:, :, 0]


def tt_to_vector(x):
    """Dense vector of a TT vector with any physical dimensions, site 1 most significant."""
    v = np.ones((1, 1))
    for c in x.ttv_vec:
        v = np.einsum("pa,iab->pib", v, c).reshape(v.shape[0] * c.shape[0], c.shape[2])
    return v[:, 0]


def nontrivial_pivots(K, first=LU_NB):
    """Number of steps j >= first of LAPACK's partially pivoted LU of K that exchange row j with another one."""
    _, piv = sla.lu_factor(np.array(K, dtype=np.float64), check_finite=False)
    j = np.arange(len(piv))
    return int(np.sum((piv != j) & (j >= first)))


class PivotLog(list):
    """One (N, exchanges at steps >= LU_NB, cond) per local system the oracle solved."""

    def beyond_first_panel(self):
        return [e for e in self if e[0] > LU_NB]

    def assert_pivots_beyond_first_panel(self, at_least):
        big = self.beyond_first_panel()
        hit = [e for e in big if e[1] > 0]
        assert len(hit) >= at_least, f"only {len(hit)} of {len(big)} local systems with N > {LU_NB} exchange a row at a step >= {LU_NB}: {self}"


@contextlib.contextmanager
def pivot_spy():
    """Records every dense local system the oracle solves inside the block: als_linsolve goes through numpy.linalg.solve, mals_ and
    dmrg_linsolve through scipy.linalg.solve on Hermitian(K) — the matrix the device's LU factors too (for dmrg_linsolve up to the
    symmetric permutation between the two orderings of the unknowns).  The log tells whether a test input makes a partially pivoted LU
    exchange rows outside its first panel; without that a green test says nothing about the interchanges."""
    log = PivotLog()
    np_solve, sla_solve = O.np.linalg.solve, O.sla.solve

    def note(K):
        K = np.asarray(K)
        if K.ndim == 2 and K.shape[0] == K.shape[1]:
            log.append((K.shape[0], nontrivial_pivots(K), float(np.linalg.cond(K))))

    def spy_np(K, b, *a, **kw):
        note(K)
        return np_solve(K, b, *a, **kw)

    def spy_sla(K, b, *a, **kw):
        note(K)
        return sla_solve(K, b, *a, **kw)

    O.np.linalg.solve, O.sla.solve = spy_np, spy_sla
    try:
        yield log
    finally:
        O.np.linalg.solve, O.sla.solve = np_solve, sla_solve


@contextlib.contextmanager
def oracle_solves_by_lu():
    """Inside the block the oracle's two-site solvers solve Hermitian(K) x = b by LAPACK's LU instead of its symmetric-indefinite
    factorisation: a second, equally valid rounding path through the same algorithm.  The distance between the two runs is the
    reference's OWN sensitivity on an input (near-degenerate singular values at a truncation make it large); a parity bar is only
    meaningful on inputs where it lies well below the bar."""
    orig = O.sla.solve
    O.sla.solve = lambda K, b, **kw: np.linalg.solve(K, b)
    try:
        yield
    finally:
        O.sla.solve = orig


def lu_pivots_longdouble(K, nb=64):
    """Pivot rows (0-based, first maximal modulus) of Gaussian elimination with partial pivoting carried out in numpy.longdouble
    (blocked right-looking, panels of nb columns: longdouble has no BLAS, the matrix product of the trailing update is what keeps it
    affordable), and the smallest relative margin (|pivot| - |runner-up|) / |pivot| over all steps: a margin far above 2^-53 times
    the growth means that no rounding path of an fp64 elimination can choose another row."""
    A = np.array(K, dtype=np.longdouble)
    n = A.shape[0]
    piv = np.zeros(n, dtype=np.int64)
    margin = np.longdouble(np.inf)
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        for j in range(k0, k1):
            col = np.abs(A[j:, j])
            p = int(np.argmax(col))
            if len(col) > 1:
                margin = min(margin, (col[p] - np.max(np.delete(col, p))) / col[p])
            piv[j] = j + p
            if p:
                A[[j, j + p], :] = A[[j + p, j], :]
            if j + 1 < n:
                A[j + 1:, j] /= A[j, j]
                A[j + 1:, j + 1:k1] -= np.outer(A[j + 1:, j], A[j, j + 1:k1])
        if k1 < n:
            for j in range(k0, k1 - 1):                                    # U12 = L11^-1 A12
                A[j + 1:k1, k1:] -= np.outer(A[j + 1:k1, j], A[j, k1:])
            A[k1:, k1:] -= A[k1:, k0:k1] @ A[k0:k1, k1:]
    return piv, float(margin)


def backward_error(K, x, b):
    """Normwise backward error ||b - K x||_inf / (||K||_inf ||x||_inf + ||b||_inf), evaluated in numpy.longdouble."""
    Kl, xl, bl = (np.array(a, dtype=np.longdouble) for a in (K, x, b))
    r = bl - Kl @ xl
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(Kl), axis=1)) * np.max(np.abs(xl)) + np.max(np.abs(bl))))


def lu_test_system(N):
    """The random normal system (K column-major, b) of size N that tests/test_gpu_lu.py solves."""
    rng = np.random.default_rng(1000 + N)
    return np.asfortranarray(rng.standard_normal((N, N))), rng.standard_normal(N)


def matrix_fingerprint(K):
    """A few numbers that identify a drawn matrix bit for bit in practice: corners, centre, the two plain sums."""
    n = K.shape[0]
    return np.array([K[0, 0], K[-1, -1], K[n // 2, n // 3], K[0, -1], float(np.sum(K)), float(np.sum(np.abs(K)))])
