"""NumPy complex128 restatements of the site-resolved measurements on ComplexF64 trains (include/ttn_zmeasure.h), no device:

    E_O[k]     = <x| O_k |x> / <x|x>
    C_PQ[i, j] = <x| P_i Q_j |x> / <x|x>

twice, independently: ``dense_*`` from the full prod n_k state vector with ``np.vdot`` and the matrices applied along tensor axes,
``chain_*`` in the three phases of the device (both environment chains, the opened states V, right-to-left walks) in einsum.
A train is a list of complex cores (n_k, r_k, r_k+1); an operator is an (n, n) array used at every site or a sequence of d arrays, real
or complex.  The first index of a matrix meets the conjugated bra."""
import numpy as np

from tests.measure_reference import CASES, full_ranks

SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
SY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
SZ = np.array([[1, 0], [0, -1]], dtype=np.complex128)
SPLUS = np.array([[0, 1], [0, 0]], dtype=np.complex128)        # |0><1|
SMINUS = SPLUS.T.copy()
I2 = np.eye(2, dtype=np.complex128)


def crand_train(dims, rks, rng):
    """Seeded random complex cores with entries (re + i im) / sqrt(2 r_left): the transfer matrices neither grow nor vanish."""
    return [(rng.standard_normal((dims[k], rks[k], rks[k + 1])) + 1j * rng.standard_normal((dims[k], rks[k], rks[k + 1]))) / np.sqrt(2 * rks[k])
            for k in range(len(dims))]


def crand_matrix(n, rng):
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def per_site(op, dims):
    a = op if isinstance(op, (list, tuple)) else np.asarray(op)
    if not isinstance(a, (list, tuple)) and a.ndim == 2:
        return [np.asarray(a, dtype=np.complex128)] * len(dims)
    mats = [np.asarray(m, dtype=np.complex128) for m in a]
    assert len(mats) == len(dims) and all(m.shape == (n, n) for m, n in zip(mats, dims))
    return mats


def op_norms(op, dims):
    """The spectral norm of every site's matrix: the scale of the tolerances."""
    return np.array([np.linalg.norm(m, 2) for m in per_site(op, dims)])


def dagger(op, dims):
    return [m.conj().T for m in per_site(op, dims)]


# ---- dense ---------------------------------------------------------------------------------------------------------------------------
def dense_vector(cores):
    psi = np.ones((1, 1), dtype=np.complex128)
    for c in cores:
        psi = np.tensordot(psi, np.asarray(c, dtype=np.complex128).transpose(1, 0, 2), axes=([psi.ndim - 1], [0]))
    return psi.reshape([c.shape[0] for c in cores])


def _apply_axis(M, psi, k):
    """out[.. z_k ..] = sum_z' M[z_k, z'] psi[.. z' ..]"""
    return np.moveaxis(np.tensordot(M, psi, axes=([1], [k])), 0, k)


def dense_site_expect(cores, op, normalize=True):
    dims = [c.shape[0] for c in cores]
    mats = per_site(op, dims)
    psi = dense_vector(cores)
    nn = np.real(np.vdot(psi, psi)) if normalize else 1.0
    return np.array([np.vdot(psi, _apply_axis(mats[k], psi, k)) / nn for k in range(len(dims))])


def dense_correlation(cores, P, Q=None, normalize=True):
    dims = [c.shape[0] for c in cores]
    d = len(dims)
    Pm, Qm = per_site(P, dims), per_site(P if Q is None else Q, dims)
    psi = dense_vector(cores)
    nn = np.real(np.vdot(psi, psi)) if normalize else 1.0
    out = np.zeros((d, d), dtype=np.complex128)
    for j in range(d):
        qpsi = _apply_axis(Qm[j], psi, j)
        for i in range(d):
            if i == j:
                out[i, j] = np.vdot(psi, _apply_axis(Pm[i] @ Qm[i], psi, i)) / nn
            else:
                out[i, j] = np.vdot(psi, _apply_axis(Pm[i], qpsi, i)) / nn
    return out


# ---- chains: the three phases of csrc/ttn_zmeasure_kernels.h -------------------------------------------------------------------------
def _lr(L, c, O=None):
    """L'[a, b] = sum conj(c[z, al, a]) L[al, be] O[z, z'] c[z', be, b]   (O = identity when None)"""
    ket = c if O is None else np.einsum("zy,ybc->zbc", O, c)
    return np.einsum("zpa,pq,zqb->ab", c.conj(), L, ket, optimize=True)


def _rl(G, c, O=None):
    """G'[al, be] = sum conj(c[z, al, a]) G[a, b] O[z, z'] c[z', be, b]"""
    ket = c if O is None else np.einsum("zy,ybc->zbc", O, c)
    return np.einsum("zpa,ab,zqb->pq", c.conj(), G, ket, optimize=True)


def chains(cores):
    """(L, G): the environments on bond 0 .. d from either end, every state kept (phase 0)."""
    cores = [np.asarray(c, dtype=np.complex128) for c in cores]
    d = len(cores)
    L = [np.ones((1, 1), dtype=np.complex128)]
    for c in cores:
        L.append(_lr(L[-1], c))
    G = [None] * (d + 1)
    G[d] = np.ones((1, 1), dtype=np.complex128)
    for k in range(d - 1, -1, -1):
        G[k] = _rl(G[k + 1], cores[k])
    return L, G


def chain_norm2(cores):
    return float(np.real(chains(cores)[0][-1][0, 0]))


def _opened(cores, L, mats):
    """V^O_k = one left-to-right site with the ket core O_k x_k on L_k (phase 1)."""
    return [_lr(L[k], cores[k], mats[k]) for k in range(len(cores))]


def chain_site_expect(cores, op, normalize=True):
    cores = [np.asarray(c, dtype=np.complex128) for c in cores]
    dims = [c.shape[0] for c in cores]
    L, G = chains(cores)
    nn = np.real(L[-1][0, 0]) if normalize else 1.0
    V = _opened(cores, L, per_site(op, dims))
    return np.array([np.sum(V[k] * G[k + 1]) / nn for k in range(len(dims))])          # the plain product: no conjugate


def chain_correlation(cores, P, Q=None, normalize=True):
    cores = [np.asarray(c, dtype=np.complex128) for c in cores]
    dims = [c.shape[0] for c in cores]
    d = len(dims)
    Pm, Qm = per_site(P, dims), per_site(P if Q is None else Q, dims)
    L, G = chains(cores)
    nn = np.real(L[-1][0, 0]) if normalize else 1.0
    out = np.zeros((d, d), dtype=np.complex128)
    VPQ = _opened(cores, L, [p @ q for p, q in zip(Pm, Qm)])
    for k in range(d):
        out[k, k] = np.sum(VPQ[k] * G[k + 1]) / nn
    # phase 2: the walk that opens at j with O1 and meets V^{O2}_i in front of every i < j
    for O1, O2, upper in ((Qm, Pm, True), (Pm, Qm, False)):
        V2 = _opened(cores, L, O2)
        for j in range(1, d):
            Tm = _rl(G[j + 1], cores[j], O1[j])
            for i in range(j - 1, -1, -1):
                v = np.sum(V2[i] * Tm) / nn
                if upper:
                    out[i, j] = v                   # <P_i Q_j>
                else:
                    out[j, i] = v                   # <P_j Q_i>
                if i > 0:
                    Tm = _rl(Tm, cores[i])
    return out


# ---- analytic trains -----------------------------------------------------------------------------------------------------------------
def plus_y_train(d):
    """|+y>^(x)d, |+y> = (|0> + i |1>) / sqrt 2: <sigma_y> = +1, <sigma_x> = <sigma_z> = 0."""
    return [(np.array([1.0, 1.0j]) / np.sqrt(2.0)).reshape(2, 1, 1) for _ in range(d)]


def precessing_train(thetas):
    """Cores exp(-i theta_k sigma_x) |up> = (cos theta_k, -i sin theta_k): <sigma_z> = cos 2 theta_k, <sigma_y> = -sin 2 theta_k."""
    return [np.array([np.cos(t), -1j * np.sin(t)]).reshape(2, 1, 1) for t in thetas]


def complex_ghz_train(d, phi):
    """(|0...0> + e^{i phi} |1...1>) / sqrt(2) as a rank-2 train of d >= 2 sites."""
    cores = []
    for k in range(d):
        rl, rr = (1 if k == 0 else 2), (1 if k == d - 1 else 2)
        c = np.zeros((2, rl, rr), dtype=np.complex128)
        for z in range(2):
            c[z, 0 if rl == 1 else z, 0 if rr == 1 else z] = 1.0
        cores.append(c)
    cores[0] = cores[0] / np.sqrt(2.0)
    cores[-1][1] = cores[-1][1] * np.exp(1j * phi)
    return cores


# ---- the shapes both test files use: those of measure_reference.CASES, complex ------------------------------------------------------------
def case(name):
    """(dims, [train, ...], P, Q) of a named case of measure_reference.CASES: seeded complex trains, complex non-Hermitian random
    P != Q (per site where the dims differ)."""
    dims, caps, seed = CASES[name]
    rng = np.random.default_rng(seed + 7)
    trains = [crand_train(dims, full_ranks(dims, cap), rng) for cap in caps]
    if len(set(dims)) == 1:
        P, Q = crand_matrix(dims[0], rng), crand_matrix(dims[0], rng)
    else:
        P, Q = [crand_matrix(n, rng) for n in dims], [crand_matrix(n, rng) for n in dims]
    return dims, trains, P, Q
