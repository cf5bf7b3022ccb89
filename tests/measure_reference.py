"""NumPy restatements of the site-resolved measurements (include/ttn_measure.h), no device:

    E_O[k]     = <x| O_k |x> / <x, x>
    C_PQ[i, j] = <x| P_i Q_j |x> / <x, x>

twice, independently: ``dense_*`` from the full prod n_k vector with the matrices applied along tensor axes, ``chain_*`` from transfer
matrices in float64, pair by pair and left to right (not the device's order: it walks right to left from stored environments).
A train is a list of cores (n_k, r_k, r_k+1); an operator is an (n, n) array used at every site or a sequence of d arrays.  The first
index of a matrix meets the bra."""
import numpy as np


def full_ranks(dims, cap):
    """[1, n_1, n_1 n_2, ...] from both ends, capped: the largest ranks a train of these dims can carry below ``cap``."""
    d = len(dims)
    left, right = [1], [1]
    for k in range(d):
        left.append(min(left[-1] * dims[k], 10 ** 9))
        right.append(min(right[-1] * dims[d - 1 - k], 10 ** 9))
    right = right[::-1]
    return [int(min(left[m], right[m], cap)) for m in range(d + 1)]


def rand_train(dims, rks, rng):
    """Seeded random cores with entries scaled by 1 / sqrt(r_left): the transfer matrices neither grow nor vanish along the chain."""
    return [rng.standard_normal((dims[k], rks[k], rks[k + 1])) / np.sqrt(rks[k]) for k in range(len(dims))]


def per_site(op, dims):
    a = op if isinstance(op, (list, tuple)) else np.asarray(op)
    if not isinstance(a, (list, tuple)) and a.ndim == 2:
        return [np.asarray(a, dtype=np.float64)] * len(dims)
    mats = [np.asarray(m, dtype=np.float64) for m in a]
    assert len(mats) == len(dims) and all(m.shape == (n, n) for m, n in zip(mats, dims))
    return mats


def op_norms(op, dims):
    """The spectral norm of every site's matrix: the scale of the tolerances."""
    return np.array([np.linalg.norm(m, 2) for m in per_site(op, dims)])


# ---- dense ---------------------------------------------------------------------------------------------------------------------------
def dense_vector(cores, dtype=np.float64):
    psi = np.ones((1, 1), dtype=dtype)
    for c in cores:
        c = np.asarray(c, dtype=dtype)
        psi = np.tensordot(psi, c.transpose(1, 0, 2), axes=([psi.ndim - 1], [0]))       # (..., n_k, r_k+1)
    return psi.reshape([c.shape[0] for c in cores])


def _apply_axis(M, psi, k):
    """out[.. z_k ..] = sum_z' M[z_k, z'] psi[.. z' ..]"""
    return np.moveaxis(np.tensordot(np.asarray(M, dtype=psi.dtype), psi, axes=([1], [k])), 0, k)


def dense_site_expect(cores, op, normalize=True, dtype=np.float64):
    dims = [c.shape[0] for c in cores]
    mats = per_site(op, dims)
    psi = dense_vector(cores, dtype)
    nn = np.sum(psi * psi) if normalize else 1
    return np.array([np.sum(psi * _apply_axis(mats[k], psi, k)) / nn for k in range(len(dims))], dtype=dtype)


def dense_correlation(cores, P, Q=None, normalize=True, dtype=np.float64):
    dims = [c.shape[0] for c in cores]
    d = len(dims)
    Pm, Qm = per_site(P, dims), per_site(P if Q is None else Q, dims)
    psi = dense_vector(cores, dtype)
    nn = np.sum(psi * psi) if normalize else 1
    out = np.zeros((d, d), dtype=dtype)
    for j in range(d):
        qpsi = _apply_axis(Qm[j], psi, j)
        for i in range(d):
            if i == j:
                out[i, j] = np.sum(psi * _apply_axis(np.asarray(Pm[i], dtype=dtype) @ np.asarray(Qm[i], dtype=dtype), psi, i)) / nn
            else:
                out[i, j] = np.sum(psi * _apply_axis(Pm[i], qpsi, i)) / nn
    return out


# ---- chains --------------------------------------------------------------------------------------------------------------------------
def _step(M, c, O=None):
    """M'[a, b] = sum_{z, z', al, be} M[al, be] c[z, al, a] O[z, z'] c[z', be, b]   (O = identity when None)"""
    ket = c if O is None else np.einsum("zy,ybc->zbc", O, c)
    return np.einsum("ab,zac,zbd->cd", M, c, ket, optimize=True)


def chain_norm2(cores):
    M = np.ones((1, 1))
    for c in cores:
        M = _step(M, c)
    return float(M[0, 0])


def _right_envs(cores):
    d = len(cores)
    R = [None] * (d + 1)
    R[d] = np.ones((1, 1))
    for k in range(d - 1, -1, -1):
        R[k] = np.einsum("zac,zbd,cd->ab", cores[k], cores[k], R[k + 1], optimize=True)
    return R


def chain_site_expect(cores, op, normalize=True):
    dims = [c.shape[0] for c in cores]
    mats = per_site(op, dims)
    R = _right_envs(cores)
    nn = chain_norm2(cores) if normalize else 1.0
    out = np.zeros(len(dims))
    M = np.ones((1, 1))
    for k, c in enumerate(cores):
        out[k] = np.sum(_step(M, c, mats[k]) * R[k + 1]) / nn
        M = _step(M, c)
    return out


def chain_correlation(cores, P, Q=None, normalize=True):
    dims = [c.shape[0] for c in cores]
    d = len(dims)
    Pm, Qm = per_site(P, dims), per_site(P if Q is None else Q, dims)
    R = _right_envs(cores)
    nn = chain_norm2(cores) if normalize else 1.0
    out = np.zeros((d, d))
    L = [np.ones((1, 1))]
    for c in cores:
        L.append(_step(L[-1], c))
    for i in range(d):
        out[i, i] = np.sum(_step(L[i], cores[i], Pm[i] @ Qm[i]) * R[i + 1]) / nn
        # the earlier site carries its operator to every later one: (first, second) = (P_i, Q_j) gives C[i, j], (Q_i, P_j) gives C[j, i]
        for first, second, transpose in ((Pm, Qm, False), (Qm, Pm, True)):
            M = _step(L[i], cores[i], first[i])
            for j in range(i + 1, d):
                v = np.sum(_step(M, cores[j], second[j]) * R[j + 1]) / nn
                if transpose:
                    out[j, i] = v
                else:
                    out[i, j] = v
                M = _step(M, cores[j])
    return out


# ---- analytic trains -----------------------------------------------------------------------------------------------------------------
def ghz_train(d):
    """(|0...0> + |1...1>) / sqrt(2) as a rank-2 train of d >= 2 sites."""
    cores = []
    for k in range(d):
        rl, rr = (1 if k == 0 else 2), (1 if k == d - 1 else 2)
        c = np.zeros((2, rl, rr))
        for z in range(2):
            c[z, 0 if rl == 1 else z, 0 if rr == 1 else z] = 1.0
        cores.append(c)
    cores[0] = cores[0] / np.sqrt(2.0)
    return cores


def product_train(dims, rng):
    return [rng.standard_normal((n, 1, 1)) for n in dims]


# ---- the shapes both test files use --------------------------------------------------------------------------------------------------
# name -> (dims, rank caps of the trains of the batch, seed)
CASES = {
    "class_d12": ((2,) * 12, (64, 13, 7), 1201),          # the LDS-resident class: full ranks 1, 2, .., 64, .., 2, 1; ragged ranks off the tile
    "rank80_d14": ((2,) * 14, (80,), 1401),               # the interior leaves the class, the ramps stay inside it
    "mixed_dims": ((2, 3, 2, 4, 3), (1000, 3), 501),      # per-site tables, the general route
    "n3_d6": ((3,) * 6, (9, 4), 601),
}


def case(name):
    """(dims, [train, ...], P, Q) of a named case: seeded trains, non-symmetric random P != Q (per site where the dims differ)."""
    dims, caps, seed = CASES[name]
    rng = np.random.default_rng(seed)
    trains = [rand_train(dims, full_ranks(dims, cap), rng) for cap in caps]
    if len(set(dims)) == 1:
        P, Q = rng.standard_normal((dims[0], dims[0])), rng.standard_normal((dims[0], dims[0]))
    else:
        P, Q = [rng.standard_normal((n, n)) for n in dims], [rng.standard_normal((n, n)) for n in dims]
    return dims, trains, P, Q
