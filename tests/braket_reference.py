"""NumPy restatement of what the braket tests need, written from the formulas:

* ``braket(x, A, y)``: <x| A |y> = sum_ij conj(x_i) A_ij y_j by the three-layer transfer recurrence of tests/expect_reference.py in
  complex128, with ``np.conj`` on x's layer,
      M_0 = [1],   M_k[a, be, b] = sum_{i, j, al, ga, bl} conj(x_k[i, al, a]) A_k[i, j, ga, be] y_k[j, bl, b] M_{k-1}[al, ga, bl],
  the result being the single entry of M_d; ``conj_x=False`` reads x as it is (the bilinear form: a different number on complex x);
* the three Pauli matrices and their sums as dense complex sums of Kronecker products (site 1 is the most significant bit, as
  qtto_to_matrix orders a matrix).
"""
import numpy as np

PAULI = {"x": np.array([[0.0, 1.0], [1.0, 0.0]], dtype=np.complex128),
         "y": np.array([[0.0, -1.0j], [1.0j, 0.0]], dtype=np.complex128),
         "z": np.array([[1.0, 0.0], [0.0, -1.0]], dtype=np.complex128)}


def braket(x, A, y, conj_x: bool = True) -> complex:
    """<x| A |y> for oracle-style trains (cores (n, r_l, r_r)) and an operator (cores (n, n, R_l, R_r), first index the output)."""
    M = np.ones((x.ttv_rks[0], A.tto_rks[0], y.ttv_rks[0]), dtype=np.complex128)
    assert M.size == 1
    for k in range(x.N):
        xk = np.asarray(x.ttv_vec[k], dtype=np.complex128)
        U = np.einsum("agb,jbB->agjB", M, np.asarray(y.ttv_vec[k], dtype=np.complex128))       # y's layer
        V = np.einsum("agjB,ijgG->aiGB", U, np.asarray(A.tto_vec[k], dtype=np.complex128))     # the operator's layer
        M = np.einsum("aiGB,iaA->AGB", V, np.conj(xk) if conj_x else xk)                       # x's layer, conjugated
    assert M.size == 1
    return complex(M.reshape(-1)[0])


def _site_product(d: int, placed: dict) -> np.ndarray:
    """I (x) ... (x) placed[k] (x) ... (x) I on d sites (0-based keys), site 0 the most significant bit."""
    out = np.ones((1, 1), dtype=np.complex128)
    for k in range(d):
        out = np.kron(out, placed.get(k, np.eye(2)))
    return out


def pauli_sum_dense(mu: str, d: int) -> np.ndarray:
    return sum(_site_product(d, {k: PAULI[mu]}) for k in range(d))


def pauli_pair_sum_dense(mu: str, nu: str, d: int) -> np.ndarray:
    return sum(_site_product(d, {k: PAULI[mu], k + 1: PAULI[nu]}) for k in range(d - 1))
