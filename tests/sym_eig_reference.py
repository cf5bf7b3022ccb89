"""NumPy restatement of the dense symmetric eigen routine of the two-site eigensolvers, wg_sym_eig_smallest (csrc/ttn_eigsolve_kernels.h),
step for step: Householder tridiagonalisation, multisection on Sturm counts at TTN_WG points per round, inverse iteration on the
tridiagonal from the fixed start vector, modified Gram-Schmidt with the restart of a collapsed vector, and the back-transformation.  It
follows the device's operations, not its reduction order, so it agrees with the device to rounding, not bitwise.  `restart=False`
gives the routine as it was before collapsed vectors were recomputed (a repeated eigenvalue then leaves a 0/0 NaN vector)."""
import numpy as np

TTN_WG = 1024
EPS = 2.220446049250313e-16
_M64 = (1 << 64) - 1


def tridiag(A):
    """(dg, e, tau, V): T = Q^T A Q, the reflector of step k in V[k + 2:, k] (unit entry at k + 1 implicit)."""
    A = np.array(A, dtype=np.float64, copy=True)
    N = A.shape[0]
    dg, e, tau = np.zeros(N), np.zeros(max(N - 1, 0)), np.zeros(max(N - 1, 0))
    for k in range(N - 2):
        x = A[k + 1:, k].copy()
        s2 = float(np.dot(x[1:], x[1:]))
        alpha = x[0]
        tk, beta, scale = 0.0, alpha, 0.0
        if s2 > 0.0:
            beta = -np.copysign(np.sqrt(alpha * alpha + s2), alpha)
            tk = (beta - alpha) / beta
            scale = 1.0 / (alpha - beta)
        v = x * scale
        v[0] = 1.0
        tau[k], e[k], dg[k] = tk, beta, A[k, k]
        if tk != 0.0:
            A22 = A[k + 1:, k + 1:]
            p = tk * (A22 @ v)
            p -= 0.5 * tk * float(p @ v) * v
            A22 -= np.outer(v, p) + np.outer(p, v)
        A[k + 2:, k] = v[1:]
    if N >= 2:
        dg[N - 2], e[N - 2] = A[N - 2, N - 2], A[N - 1, N - 2]
        tau[N - 2] = 0.0
    dg[N - 1] = A[N - 1, N - 1]
    return dg, e, tau, A


def sturm_count(dg, e, x, pivmin):
    """Eigenvalues below each point of x (an array), the device's LDL^T pivots with vanishing ones replaced by -pivmin."""
    with np.errstate(over="ignore"):                         # 1e100-scaled inputs: e^2 / pivmin is +-inf, as on the device
        return _sturm_count(dg, e, x, pivmin)


def _sturm_count(dg, e, x, pivmin):
    q = dg[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    c = (q < 0.0).astype(np.int64)
    for i in range(1, len(dg)):
        q = (dg[i] - x) - e[i - 1] * (e[i - 1] / q)
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        c += q < 0.0
    return c


def tri_eigval(dg, e, j):
    N = len(dg)
    r = np.zeros(N)
    if N > 1:
        r[1:] += np.abs(e)
        r[:-1] += np.abs(e)
    lo, hi, tn = float(np.min(dg - r)), float(np.max(dg + r)), float(np.max(np.abs(dg) + r))
    pivmin = max(tn * 1.0e-300, 2.2250738585072014e-308)
    lo -= 2.0 * EPS * tn + pivmin
    hi += 2.0 * EPS * tn + pivmin
    for _ in range(12):
        if hi - lo <= 2.0 * EPS * max(abs(lo), abs(hi)) + pivmin:
            break
        step = (hi - lo) / (TTN_WG + 1)
        x = lo + (np.arange(TTN_WG) + 1) * step
        above = sturm_count(dg, e, x, pivmin) > j
        if np.any(~above):
            lo = max(lo, float(np.max(x[~above])))
        if np.any(above):
            hi = min(hi, float(np.min(x[above])))
    return 0.5 * (lo + hi)


def tri_factor(dg, e, lam):
    """Gaussian elimination with partial pivoting of T - lam I as tri_inverse_iteration does it: (u0, u1, u2, l, sw)."""
    N = len(dg)
    r = np.zeros(N)
    if N > 1:
        r[1:] += np.abs(e)
        r[:-1] += np.abs(e)
    tn = float(np.max(np.abs(dg) + r))
    tiny = max(tn * EPS, 1.0e-300)
    u0, u1, u2, l, sw = (np.zeros(N) for _ in range(5))
    dc, fc = dg[0] - lam, (e[0] if N > 1 else 0.0)
    for i in range(N - 1):
        sub, an, ns = e[i], dg[i + 1] - lam, (e[i + 1] if i + 2 < N else 0.0)
        if abs(dc) >= abs(sub):
            piv = np.copysign(tiny, dc) if abs(dc) < tiny else dc
            m = sub / piv
            u0[i], u1[i], u2[i], l[i], sw[i] = piv, fc, 0.0, m, 0.0
            dc, fc = an - m * fc, ns
        else:
            m = dc / sub
            u0[i], u1[i], u2[i], l[i], sw[i] = sub, an, ns, m, 1.0
            dc, fc = fc - m * an, -m * ns
    u0[N - 1] = np.copysign(tiny, dc) if abs(dc) < tiny else dc
    return u0, u1, u2, l, sw


def _solve_normalise(F, y):
    u0, u1, u2, l, sw = F
    N = len(y)
    for i in range(N - 1):
        if sw[i] != 0.0:
            y[i], y[i + 1] = y[i + 1], y[i]
        y[i + 1] -= l[i] * y[i]
    for i in range(N - 1, -1, -1):
        a = y[i]
        if i + 1 < N:
            a -= u1[i] * y[i + 1]
        if i + 2 < N:
            a -= u2[i] * y[i + 2]
        y[i] = a / u0[i]
    y /= np.max(np.abs(y))
    y *= 1.0 / np.sqrt(float(y @ y))


def restart_entry(i, j):
    """tri_restart_entry: splitmix64 of (j, i) as a uniform double in [-1, 1)."""
    z = (((j + 1) << 32) + i + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return float(z >> 11) * 2.0 ** -52 - 1.0


def _mgs(Y, j, y):
    for q in range(j):
        y -= float(Y[:, q] @ y) * Y[:, q]


def sym_eig_smallest(A, k, restart=True):
    """(lam[k], Y[N, k]) of wg_sym_eig_smallest: the k smallest eigenvalues ascending and orthonormal vectors, no sign normalisation."""
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    if N == 1:
        return np.array([A[0, 0]]), np.ones((1, 1))
    dg, e, tau, V = tridiag(A)
    lam = np.array([tri_eigval(dg, e, j) for j in range(k)])
    F = [tri_factor(dg, e, lam[j]) for j in range(k)]
    Y = np.zeros((N, k))
    for j in range(k):
        y = 1.0 + 0.5 * np.sin(1.0 + 0.7 * np.arange(N))
        for _ in range(3):
            _solve_normalise(F[j], y)
        Y[:, j] = y
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(1, k):
            y = Y[:, j]
            _mgs(Y, j, y)
            s = float(y @ y)
            if restart and not s >= 0.25:
                y[:] = [restart_entry(i, j) for i in range(N)]
                for _ in range(3):
                    _mgs(Y, j, y)
                    _mgs(Y, j, y)
                    _solve_normalise(F[j], y)
                _mgs(Y, j, y)
                _mgs(Y, j, y)
                s = float(y @ y)
            y *= 1.0 / np.sqrt(s)
    for j in range(k):                                      # y <- H_0 ... H_{N-3} y
        y = Y[:, j]
        for kk in range(N - 3, -1, -1):
            if tau[kk] == 0.0:
                continue
            v = np.concatenate(([1.0], V[kk + 2:, kk]))
            y[kk + 1:] -= tau[kk] * float(v @ y[kk + 1:]) * v
    return lam, Y


# ---- test matrices and the checks both the CPU and the GPU tests apply ----

def _orth(N, rng):
    q, r = np.linalg.qr(rng.standard_normal((N, N)))
    return q * np.sign(np.diag(r))


def _spectrum(N, Q, lam):
    return (Q * lam) @ Q.T


def wilkinson_plus(m=10):
    """W_{2m+1}^+: diagonal |m - i|, unit off-diagonals (its largest eigenvalues come in pairs closer than 1e-13)."""
    return np.diag(np.abs(np.arange(2 * m + 1) - m).astype(float)) + np.diag(np.ones(2 * m), 1) + np.diag(np.ones(2 * m), -1)


def families(N, rng, heavy=True):
    """[(name, A)]: the symmetric test matrices of size N.  heavy=False: a cheaper subset for the largest sizes."""
    out = []
    B = rng.standard_normal((N, N))
    out.append(("random", 0.5 * (B + B.T)))
    d = rng.permutation(N).astype(float) + 1.0
    out.append(("diag_distinct", np.diag(d)))
    if N >= 2:
        dr = d.copy()
        dr[dr == 2.0] = 1.0                                  # smallest entry twice
        out.append(("diag_repeated2", np.diag(dr)))
    if N >= 6:
        out.append(("diag_112345", np.diag(np.concatenate(([1.0, 1.0, 2.0, 3.0, 4.0, 5.0], 6.0 + np.arange(N - 6))))))
    out.append(("zero", np.zeros((N, N))))
    out.append(("cI", 2.5 * np.eye(N)))
    if N >= 4:
        Q = _orth(N, rng)
        base = 1.0 + rng.random(N)
        for mult in (2, 3):
            lam = base.copy()
            lam[:mult] = 0.25
            out.append(("mult%d" % mult, _spectrum(N, Q, lam)))
        gaps = (1e-6, 1e-10, 1e-14) if heavy else (1e-10,)
        for g in gaps:
            lam = base.copy()
            lam[:3] = 0.25 + g * np.arange(3)
            out.append(("cluster%.0e" % g, _spectrum(N, Q, lam)))
    if not heavy:
        return out
    m = next((m for m in (4, 3, 2) if N % m == 0 and N > m), 0)
    if m:                                                    # every eigenvalue m-fold
        blk = rng.standard_normal((N // m, N // m))
        out.append(("block_identical", np.kron(np.eye(m), 0.5 * (blk + blk.T))))
    if N >= 3:
        th = np.sort(rng.standard_normal(N - 1))
        th[1] = th[0]                                        # a repeated Ritz value, as after locked ones
        for bscale in (1.0, 1e-16):
            A = np.diag(np.concatenate((th, [rng.standard_normal()])))
            A[:-1, -1] = A[-1, :-1] = bscale * rng.standard_normal(N - 1)
            out.append(("arrow_b%.0e" % bscale, A))
        off = 10.0 ** rng.uniform(-15, 0, N - 1)
        T = np.diag(rng.standard_normal(N)) + np.diag(off, 1) + np.diag(off, -1)
        out.append(("tridiag_small_offdiag", T))
        D = np.logspace(-4, 4, N)
        out.append(("graded", (D[:, None] * 0.5 * (B + B.T)) * D[None, :]))
        out.append(("neg_definite", -(B @ B.T / N + np.eye(N))))
    return out


def check_eigpairs(A, k, lam, Y, tol, w=None, U=None):
    """Eigenvalues against numpy.linalg.eigh, residuals ||A y_j - lam_j y_j|| and orthogonality of Y (all absolute, relative to ||A||_2),
    and every vector against eigh's invariant subspace of its cluster (eigenvalues within 1e-5 ||A||) by the Davis-Kahan bound
    sin(angle) <= residual / gap.  Returns a message for the first violation, or None."""
    N = A.shape[0]
    if w is None:
        w, U = np.linalg.eigh(A)
    nrm = max(float(np.max(np.abs(w))), 1e-280)              # the zero matrix: the multisection bracket keeps a pivmin-wide floor
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(Y))):
        return "non-finite output"
    err = float(np.max(np.abs(lam - w[:k])))
    if err > tol * nrm:
        return "eigenvalue error %.3e > %.1e * %.3e" % (err, tol, nrm)
    R = A @ Y - Y * lam
    res = float(np.max(np.linalg.norm(R, axis=0)))
    if res > tol * nrm:
        return "residual %.3e > %.1e * %.3e" % (res, tol, nrm)
    orth = float(np.max(np.abs(Y.T @ Y - np.eye(k))))
    if orth > tol:
        return "orthogonality %.3e > %.1e" % (orth, tol)
    for j in range(k):
        S = np.abs(w - w[j]) <= 1e-5 * nrm
        if np.all(S):
            continue
        gap = float(np.min(np.abs(w[~S] - w[j])))
        y = Y[:, j]
        s = float(np.linalg.norm(y - U[:, S] @ (U[:, S].T @ y)))
        if s > 4.0 * tol * nrm / gap + 4.0 * tol:
            return "vector %d leaves its invariant subspace: sin %.3e (gap %.3e)" % (j, s, gap)
    return None
