"""The device TDVP sweeps (tensortrainnumerics.jl_amd/tdvp.py: tdvp1sweep_, tdvp2sweep_) against answers that do not depend on the
oracle, and against the oracle over the whole real / complex dtype matrix.

* Exactness.  At saturated bond dimensions (1, 2, 4, ..., 2^{d/2}, ..., 2, 1), with truncerr = 0 and unbounded max_bond, one two-site
  sweep is exp(-i dt H) ψ to rounding.  H is an Ising chain with a y field (complex Hermitian, H != H^T), so a device path that swapped
  s and s' would evolve under H^T = conj(H) and land 1e-2 .. 1e-1 away; the bar is 1e-10.
* Invariants.  The one-site sweep is not exact (full dt in both directions, as the reference integrates), but for real dt and a
  Hermitian H it conserves the norm and <ψ|H|ψ> exactly.
* The dtype matrix.  Real / complex ψ x real / complex-typed / complex H x real / imaginary / complex dt, both sweeps, then a second
  sweep with the carried environments: the device equals the oracle, or both raise TTNError (a real ψ cannot hold a complex result:
  Julia's InexactError on the store into ψ's arrays) and ψ is unchanged.  Real ψ, real H, dt = 0.02im runs the real (cplx = 0) kernels.
* Rank-deficient splits.  qtt_sin zero-padded to saturated bonds: exact zero singular values in every two-site block.  The sites the
  sweep returns must be isometries (the SVD completes U to an orthonormal set, as LAPACK does), so a further sweep is again exact.

Dense reference: the operator as O.tto_to_tensor(H).reshape(2^d, 2^d, order="F") acting on O.ttv_to_tensor(ψ).reshape(-1, order="F")
(site 1 the fastest index), checked against O.apply in test_dense_convention (CPU); scipy.sparse builds the same matrix from its
Pauli terms for d = 12."""
import math

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
from scipy.sparse.linalg import expm_multiply

from oracle import tt_oracle as O
from helpers import to_oracle, to_product

gpu = pytest.mark.gpu

I2 = np.eye(2, dtype=complex)
PX = np.array([[0, 1], [1, 0]], dtype=complex)
PY = np.array([[0, -1j], [1j, 0]])
PZ = np.diag([1.0, -1.0]).astype(complex)
J_, H_, G_ = 1.0, 0.7, 0.4


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def ising_y(d, J=J_, h=H_, g=G_):
    """J sum Z_k Z_{k+1} + sum (h Y_k + g X_k) as a rank-3 MPO: W[0,0] = I, W[0,1] = Z, W[0,2] = hY + gX, W[1,2] = JZ, W[2,2] = I;
    cores (s_out, s_in, a, b)."""
    W = np.zeros((3, 3, 2, 2), dtype=complex)
    W[0, 0], W[0, 1], W[0, 2], W[1, 2], W[2, 2] = I2, PZ, h * PY + g * PX, J * PZ, I2
    cores = []
    for k in range(d):
        w = W[:1] if k == 0 else W
        w = w[:, 2:] if k == d - 1 else w
        cores.append(np.ascontiguousarray(np.transpose(w, (2, 3, 0, 1))))
    return O.TToperator(d, cores, (2,) * d, [1] + [3] * (d - 1) + [1], [0] * d)


def ising_y_sparse(d, J=J_, h=H_, g=G_):
    """the same operator from its Pauli terms; site k (0-based) is the k-th fastest index of the column-major vector"""
    def at(ops):                                                   # ops: {site: 2x2}
        M = sp.identity(1, dtype=complex, format="csr")
        for k in range(d - 1, -1, -1):
            M = sp.kron(M, sp.csr_matrix(ops.get(k, I2)), format="csr")
        return M
    H = sum(J * at({k: PZ, k + 1: PZ}) for k in range(d - 1))
    return (H + sum(at({k: h * PY + g * PX}) for k in range(d))).tocsr()


def conj_op(H):
    return O.TToperator(H.N, [np.conj(c) for c in H.tto_vec], tuple(H.tto_dims), list(H.tto_rks), list(H.tto_ot))


def dense_op(H):
    return O.tto_to_tensor(H).reshape(2 ** H.N, 2 ** H.N, order="F")


def dense_vec(x):
    return O.ttv_to_tensor(to_oracle(x)).reshape(-1, order="F")


def saturated(d):
    return [min(2 ** k, 2 ** (d - k)) for k in range(d + 1)]


def rand_state(d, seed, cplx=True, rks=None):
    """random train (ranks saturated unless given), orthogonalized to centre 1 (the sweeps' starting gauge) and normalised"""
    rng = np.random.default_rng(seed)
    rks = saturated(d) if rks is None else rks
    x = O.rand_tt((2,) * d, rks, rng)
    if cplx:
        y = O.rand_tt((2,) * d, rks, rng)
        x = O.TTvector(d, [a + 1j * b for a, b in zip(x.ttv_vec, y.ttv_vec)], x.ttv_dims, list(x.ttv_rks), [0] * d)
    x = O.orthogonalize(x)
    return O.scale(1.0 / O.norm(x), x)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_dense_convention():
    """the dense reference's index order: (dense H)(dense ψ) is the dense tensor of O.apply(H, ψ); the sparse build is the same matrix"""
    d = 6
    H = ising_y(d)
    x = rand_state(d, 5, rks=[1, 2, 3, 3, 3, 2, 1])
    assert rel(dense_op(H) @ dense_vec(x), dense_vec(O.apply(H, x))) < 1e-13
    assert abs(ising_y_sparse(d) - sp.csr_matrix(dense_op(H))).max() < 1e-14
    Hd = dense_op(H)
    assert np.allclose(Hd, Hd.conj().T, atol=1e-14) and np.linalg.norm(Hd - Hd.T) > 1.0       # Hermitian, not symmetric


# ---- exactness of one two-site sweep at saturated bonds ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [6, 8, 10])
@pytest.mark.parametrize("dt", [0.01, 0.05, 0.02j])
def test_tdvp2sweep_is_exact_at_saturated_bonds(T, d, dt):
    H = ising_y(d)
    psi = rand_state(d, 300 + d)
    v0 = dense_vec(psi)
    Hd = dense_op(H)
    exact = sla.expm(-1j * dt * Hd) @ v0
    wrong = sla.expm(-1j * dt * Hd.conj()) @ v0                       # what an s <-> s' transposition would evolve under
    assert rel(wrong, exact) > 1e-3
    got, F = T.tdvp.tdvp2sweep_(dt, to_product(O.copy_tt(psi)), to_product(H), None, max_bond=2 ** 62, truncerr=0.0)
    assert got.ttv_rks == saturated(d) and len(F) == d + 2
    assert np.iscomplexobj(got.ttv_vec[0])
    assert rel(dense_vec(got), exact) <= 1e-10


@gpu
def test_tdvp2sweep_is_exact_at_bond_64(T):
    """d = 12: bond 64, so the middle two-site blocks are 128 x 128 (the SVD and the H2 contraction at TDVP sizes)"""
    d, dt = 12, 0.03
    psi = rand_state(d, 412)
    v0 = dense_vec(psi)
    Hs = ising_y_sparse(d)
    exact = expm_multiply(-1j * dt * Hs, v0)
    wrong = expm_multiply(-1j * dt * Hs.conj(), v0)
    assert rel(wrong, exact) > 1e-3
    got, _ = T.tdvp.tdvp2sweep_(dt, to_product(O.copy_tt(psi)), to_product(ising_y(d)), None)
    assert got.ttv_rks == saturated(d)
    assert rel(dense_vec(got), exact) <= 1e-10


# ---- invariants of the one-site sweep ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d,r,dt", [(6, None, 0.05), (8, 5, 0.1), (10, 32, 0.05)])
def test_tdvp1sweep_conserves_norm_and_energy(T, d, r, dt):
    H = ising_y(d)
    rks = None if r is None else [min(r, 2 ** k, 2 ** (d - k)) for k in range(d + 1)]
    psi = rand_state(d, 500 + d, rks=rks)
    Hd = dense_op(H)
    v0 = dense_vec(psi)
    e0 = np.vdot(v0, Hd @ v0).real
    got, F = T.tdvp.tdvp1sweep_(dt, to_product(O.copy_tt(psi)), to_product(H), None)
    assert got.ttv_rks == psi.ttv_rks
    v1 = dense_vec(got)
    assert abs(np.linalg.norm(v1) - np.linalg.norm(v0)) <= 1e-11 * np.linalg.norm(v0)
    assert abs(np.vdot(v1, Hd @ v1).real - e0) <= 1e-11 * max(abs(e0), np.linalg.norm(Hd @ v0))
    assert rel(v1, v0) > 1e-3                                            # (it moved)
    # a second sweep with the carried environments: still conserved
    got2, _ = T.tdvp.tdvp1sweep_(dt, got, to_product(H), F)
    v2 = dense_vec(got2)
    assert abs(np.linalg.norm(v2) - np.linalg.norm(v0)) <= 1e-11 * np.linalg.norm(v0)
    assert abs(np.vdot(v2, Hd @ v2).real - e0) <= 1e-11 * max(abs(e0), np.linalg.norm(Hd @ v0))


# ---- the dtype matrix against the oracle -------------------------------------------------------------------------------------------
def _hamiltonian(kind, d):
    if kind == "lap":
        return O.tto_scale(0.3, O.Delta(d))
    if kind == "lap_c":
        return O._tdvp_complex_op(O.tto_scale(0.3, O.Delta(d)))
    return ising_y(d)


def _raises(psi_real, hkind, dt):
    """the rule: a real ψ takes the result only when it is real, i.e. exp(-i dt H) is real: dt imaginary and H real-valued"""
    return psi_real and not (complex(dt).real == 0.0 and hkind != "ising_y")


@gpu
@pytest.mark.parametrize("sweep", ["tdvp1sweep_", "tdvp2sweep_"])
@pytest.mark.parametrize("dt", [0.05, 0.02j, 0.04 + 0.02j])
@pytest.mark.parametrize("hkind", ["lap", "lap_c", "ising_y"])
@pytest.mark.parametrize("cplx", [False, True])
def test_sweep_dtype_matrix_vs_oracle(T, sweep, dt, hkind, cplx):
    d = 5
    H = _hamiltonian(hkind, d)
    psi = rand_state(d, 700 + 10 * cplx, cplx=cplx, rks=[1, 2, 3, 3, 2, 1])
    kw = dict(max_bond=2 ** 62, truncerr=0.0) if sweep == "tdvp2sweep_" else {}
    dev, ora = getattr(T.tdvp, sweep), getattr(O, sweep)
    if _raises(not cplx, hkind, dt):
        p_dev, p_ora = to_product(O.copy_tt(psi)), O.copy_tt(psi)
        with pytest.raises(T.TTNError, match="InexactError"):
            dev(dt, p_dev, to_product(H), None, **kw)
        with pytest.raises(O.TTNError, match="InexactError"):
            ora(dt, p_ora, H, None, **kw)
        for p in (p_dev, p_ora):                                         # ψ as it was
            assert p.ttv_rks == psi.ttv_rks and all(np.array_equal(a, b) for a, b in zip(p.ttv_vec, psi.ttv_vec))
            assert all(a.dtype == np.float64 for a in p.ttv_vec)
        return
    ref, Fref = ora(dt, O.copy_tt(psi), H, None, **kw)
    got, F = dev(dt, to_product(O.copy_tt(psi)), to_product(H), None, **kw)
    want = np.complex128 if cplx else np.float64
    assert all(np.asarray(c).dtype == want for c in got.ttv_vec) and all(c.dtype == want for c in ref.ttv_vec)
    assert got.ttv_rks == ref.ttv_rks and len(F) == d + 2
    assert rel(dense_vec(got), dense_vec(ref)) <= 1e-9
    ref2, _ = ora(dt, ref, H, Fref, **kw)
    got2, _ = dev(dt, got, to_product(H), F, **kw)
    assert all(np.asarray(c).dtype == want for c in got2.ttv_vec)
    assert got2.ttv_rks == ref2.ttv_rks
    assert rel(dense_vec(got2), dense_vec(ref2)) <= 1e-9


@gpu
@pytest.mark.parametrize("sweep", ["tdvp1sweep_", "tdvp2sweep_"])
def test_real_state_zero_mpo_on_the_device(T, sweep):
    """test/test_tdvp.jl:132-145 on the device: tdvp1sweep!(0.05, ψ, 0·id, nothing) with a real ψ returns a real ψ equal to ψ0
    (the reference's bar 1e-6; the identity holds to rounding)"""
    d = 4
    psi0 = O.orthogonalize(O.qtt_sin(d, lam=math.pi))
    got, F = getattr(T.tdvp, sweep)(0.05, to_product(O.copy_tt(psi0)), to_product(O.tto_scale(0.0, O.id_tto(d))), None)
    assert got.ttv_dims == psi0.ttv_dims and len(F) == d + 2
    assert all(np.asarray(c).dtype == np.float64 for c in got.ttv_vec)
    v, v0 = dense_vec(got), dense_vec(psi0)
    assert np.isfinite(np.linalg.norm(v)) and rel(v, v0) < 1e-6 and rel(v, v0) < 1e-12


# ---- isometry after rank-deficient splits ------------------------------------------------------------------------------------------
def padded_sin(d, cplx):
    """qtt_sin(d, λ = π) orthogonalized (ranks 2), every core zero-padded to the saturated ranks: the padded slices are exactly zero"""
    x = O.orthogonalize(O.qtt_sin(d, lam=math.pi))
    R = saturated(d)
    cores = []
    for k, c in enumerate(x.ttv_vec):
        p = np.zeros((2, R[k], R[k + 1]), dtype=complex if cplx else float)
        p[:, : c.shape[1], : c.shape[2]] = c * ((0.6 + 0.8j) if (cplx and k == 0) else 1.0)
        cores.append(p)
    return O.TTvector(d, cores, (2,) * d, R, [0] * d)


@gpu
@pytest.mark.parametrize("d", [6, 8])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("hkind", ["zero", "lap"])
def test_tdvp2sweep_sites_are_isometries_after_zero_singular_values(T, d, cplx, hkind):
    H = O.tto_scale(0.0, O.id_tto(d)) if hkind == "zero" else O.tto_scale(0.3, O.Delta(d))
    dt = 0.05 if cplx else 0.02j                                          # (a real ψ takes only a real result: imaginary time)
    psi = padded_sin(d, cplx)
    ref, _ = O.tdvp2sweep_(dt, O.copy_tt(psi), H, None)
    got, _ = T.tdvp.tdvp2sweep_(dt, to_product(O.copy_tt(psi)), to_product(H), None, max_bond=2 ** 62, truncerr=0.0)
    assert got.ttv_rks == ref.ttv_rks == saturated(d)
    assert rel(dense_vec(got), dense_vec(ref)) <= 1e-9
    for k in range(1, d):                                                # sum_{s,b} A[a,s,b] conj(A[a',s,b]) = delta
        A = np.asarray(got.ttv_vec[k])                                   # (s, a, b)
        G = np.einsum("sab,scb->ac", A, A.conj())
        assert np.max(np.abs(G - np.eye(A.shape[1]))) <= 1e-12, (k, np.max(np.abs(G - np.eye(A.shape[1]))))
    # from that gauge, a further sweep under H_y is exact again
    Hy = ising_y(d)
    start = got if cplx else to_product(O._tdvp_complex(to_oracle(got)))
    v1 = dense_vec(start)
    exact = sla.expm(-1j * 0.05 * dense_op(Hy)) @ v1
    got2, _ = T.tdvp.tdvp2sweep_(0.05, start, to_product(Hy), None)
    assert rel(dense_vec(got2), exact) <= 1e-10
