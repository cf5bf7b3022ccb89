"""NumPy restatement of what the expectation-value tests need, written from the formulas:

* ``sandwich(x, A, y)``: <x, A y> by the three-layer transfer recurrence in float64,
      M_0 = [1],   M_k[a, be, b] = sum_{i, j, al, ga, bl} x_k[i, al, a] A_k[i, j, ga, be] y_k[j, bl, b] M_{k-1}[al, ga, bl],
  the result being the single entry of M_d;
* the Pauli sums as dense sums of Kronecker products (site 1 is the most significant bit, as qtto_to_matrix orders a matrix);
* the periodic transverse-field Ising matrix and the z-magnetisation of examples/ising_model.jl on a dense state.
"""
import numpy as np

PAULI = {"x": np.array([[0.0, 1.0], [1.0, 0.0]]), "z": np.array([[1.0, 0.0], [0.0, -1.0]])}
Y_REAL = np.array([[0.0, -1.0], [1.0, 0.0]])                 # sigma_y = i Y_REAL, so sigma_y (x) sigma_y = -(Y_REAL (x) Y_REAL)


def sandwich(x, A, y) -> float:
    """<x, A y> for oracle-style trains (cores (n, r_l, r_r)) and an operator (cores (n, n, R_l, R_r), first index the output)."""
    M = np.ones((x.ttv_rks[0], A.tto_rks[0], y.ttv_rks[0]))
    assert M.size == 1
    for k in range(x.N):
        U = np.einsum("agb,jbB->agjB", M, np.asarray(y.ttv_vec[k], dtype=np.float64))          # y's layer
        V = np.einsum("agjB,ijgG->aiGB", U, np.asarray(A.tto_vec[k], dtype=np.float64))        # the operator's layer
        M = np.einsum("aiGB,iaA->AGB", V, np.asarray(x.ttv_vec[k], dtype=np.float64))          # x's layer
    assert M.size == 1
    return float(M.reshape(-1)[0])


def _site_product(d: int, placed: dict) -> np.ndarray:
    """I (x) ... (x) placed[k] (x) ... (x) I on d sites (0-based keys), site 0 the most significant bit."""
    out = np.ones((1, 1))
    for k in range(d):
        out = np.kron(out, placed.get(k, np.eye(2)))
    return out


def pauli_sum_dense(mu: str, d: int) -> np.ndarray:
    return sum(_site_product(d, {k: PAULI[mu]}) for k in range(d))


def pauli_pair_sum_dense(mu: str, nu: str, d: int) -> np.ndarray:
    if (mu, nu) == ("y", "y"):
        return sum(_site_product(d, {k: -Y_REAL, k + 1: Y_REAL}) for k in range(d - 1))
    return sum(_site_product(d, {k: PAULI[mu], k + 1: PAULI[nu]}) for k in range(d - 1))


def periodic_ising_dense(d: int, g: float) -> np.ndarray:
    """H = -sum_k Z_k Z_{k+1} - Z_d Z_1 - g sum_k X_k."""
    Z = PAULI["z"]
    return -(pauli_pair_sum_dense("z", "z", d) + _site_product(d, {0: Z, d - 1: Z})) - g * pauli_sum_dense("x", d)


def z_magnetization(psi: np.ndarray) -> float:
    """|sum_s p(s) (1/d) sum_k (+1 if bit k of s is 0 else -1)| with p = |psi|^2 / sum |psi|^2, site 1 the most significant bit."""
    psi = np.asarray(psi, dtype=np.float64).reshape(-1)
    d = int(round(np.log2(psi.size)))
    p = psi * psi
    p = p / p.sum()
    s = np.arange(psi.size)
    spin_sum = sum(1.0 - 2.0 * ((s >> (d - 1 - k)) & 1) for k in range(d))
    return abs(float(np.sum(p * spin_sum / d)))
