"""CPU checks of the eigensolver feature: the spin-chain constructors against dense Kronecker sums of Pauli matrices, the NumPy
restatement (tests/eig_reference.py) against exact answers and the reference's own assertions (test/test_dmrg.jl:100-171 without the
N = 1 case, test/test_mals.jl:79-160), and the refusals that come back before anything reaches a device."""
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product

X = np.array([[0.0, 1.0], [1.0, 0.0]])
Y = np.array([[0.0, -1j], [1j, 0.0]])
Z = np.array([[1.0, 0.0], [0.0, -1.0]])


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def _site_op(P, k, d):
    out = np.ones((1, 1))
    for j in range(d):
        out = np.kron(out, P if j == k else np.eye(2))
    return out


def _dense_xyz(d, jx, jy, jz, lam, F):
    H = np.zeros((2 ** d, 2 ** d), dtype=complex)
    for k in range(d - 1):
        for c, P in ((jx, X), (jy, Y), (jz, Z)):
            H += c * _site_op(P, k, d) @ _site_op(P, k + 1, d)
    for k in range(d):
        H += lam * _site_op(F, k, d)
    assert np.max(np.abs(H.imag)) == 0.0
    return H.real


def _spd(d, shift=3.0):                                     # dmrg_spd_op / mals_spd_op (test_dmrg.jl:18, test_mals.jl:15)
    return O.tto_add(O.Delta(d), O.tto_scale(shift, O.id_tto(d)))


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("jx,jy,jz,lam,field", [(1.0, 1.0, 1.0, 0.0, "x"), (0.3, -0.7, 1.1, 0.4, "x"), (1.0, 0.5, -2.0, 1.3, "z"),
                                                (0.0, 2.0, 0.0, 0.0, "y")])
def test_heisenberg_xyz_dense(T, d, jx, jy, jz, lam, field):
    A = to_oracle(T.heisenberg_xyz_tto(d, jx=jx, jy=jy, jz=jz, lam=lam, field=field))
    assert A.tto_rks == [1] + [5] * (d - 1) + [1]
    F = {"x": X, "y": Y, "z": Z}[field]
    assert np.max(np.abs(O.qtto_to_matrix(A) - _dense_xyz(d, jx, jy, jz, lam, F))) <= 1e-14


@pytest.mark.parametrize("d", [2, 4, 6])
def test_ising_xxz_xxx_dense(T, d):
    for axis, P in (("x", X), ("y", Y), ("z", Z)):
        got = O.qtto_to_matrix(to_oracle(T.ising_tto(d, J=0.7, h=1.5, interaction=axis, field="x")))
        c = {"x": (0.7, 0, 0), "y": (0, 0.7, 0), "z": (0, 0, 0.7)}[axis]
        assert np.max(np.abs(got - _dense_xyz(d, *c, 1.5, X))) <= 1e-14
    got = O.qtto_to_matrix(to_oracle(T.xxz_tto(d, J=0.9, Delta=-1.7, h=0.4)))
    assert np.max(np.abs(got - _dense_xyz(d, 0.9, 0.9, 0.9 * -1.7, 0.4, Z))) <= 1e-14
    got = O.qtto_to_matrix(to_oracle(T.xxx_tto(d, J=1.2, h=-0.3, field="x")))
    assert np.max(np.abs(got - _dense_xyz(d, 1.2, 1.2, 1.2, -0.3, X))) <= 1e-14


def test_complex_field_refused(T):
    with pytest.raises(T.TTNError):
        T.heisenberg_xyz_tto(4, lam=0.5, field="y")
    with pytest.raises(T.TTNError):
        T.ising_tto(4, h=1.0, field="y")


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("d", [3, 5, 8])
def test_restatement_exact(T, mode, d):
    rng = np.random.default_rng(d + 10 * mode)
    ops = [_spd(d, 0.5), to_oracle(T.ising_tto(d, J=1.0, h=1.5))]
    if d % 2 == 0:
        ops.append(to_oracle(T.xxx_tto(d)))
    for A in ops:
        x0 = O.rand_tt((2,) * d, 2, rng)
        E, x, r = ER.two_site_eigsolve(mode, A, x0, tol=1e-13, sweep_schedule=[4], rmax_schedule=[2 ** (d // 2)])
        ev = np.linalg.eigvalsh(O.qtto_to_matrix(A))[0]
        assert abs(E[-1] - ev) <= 1e-10 * max(1.0, abs(ev))
        assert abs(np.linalg.norm(O.ttv_to_tensor(x)) - 1.0) <= 1e-12


def test_restatement_dmrg_reference_assertions():
    """test/test_dmrg.jl:100-171 (N = 2 cases)."""
    rng = np.random.default_rng(7)
    d = 4
    x0 = O.rand_tt((2,) * d, [1, 2, 2, 2, 1], rng)
    E, x, r = ER.dmrg_eigsolve(_spd(d), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert isinstance(E[0], float) and all(isinstance(v, int) for v in r) and len(E) == len(r)
    assert x.N == d and tuple(x.ttv_dims) == (2,) * d
    A = _spd(d, 3.0)
    E, x, _ = ER.dmrg_eigsolve(A, x0, sweep_schedule=[4], rmax_schedule=[4])
    rq = O.dot(x, O.apply(A, x)) / O.dot(x, x)
    assert E[-1] > 0 and math.isclose(rq, E[-1], rel_tol=0.1)
    x1 = O.rand_tt((2,) * d, [1] * 5, rng)
    E, x, r = ER.dmrg_eigsolve(_spd(d, 2.0), x1, sweep_schedule=[2, 4], rmax_schedule=[2, 4])
    assert len(E) >= 2 and max(x.ttv_rks) <= 4
    E, _, _ = ER.dmrg_eigsolve(_spd(d, 1.0), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert all(np.isfinite(E))
    x3 = O.rand_tt((2,) * 3, [1, 2, 2, 1], rng)
    E, x, r = ER.dmrg_eigsolve(_spd(3, 2.0), x3, sweep_schedule=[1], rmax_schedule=[2], it_solver=True, itslv_thresh=1, linsolv_maxiter=20)
    assert all(np.isfinite(E)) and len(r) == len(E)


def test_restatement_mals_reference_assertions():
    """test/test_mals.jl:79-160."""
    rng = np.random.default_rng(8)
    d = 4
    x0 = O.rand_tt((2,) * d, [1, 2, 2, 2, 1], rng)
    E, x, r = ER.mals_eigsolve(_spd(d), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert len(E) == len(r) and x.N == d and tuple(x.ttv_dims) == (2,) * d
    A = _spd(d, 3.0)
    E, x, _ = ER.mals_eigsolve(A, x0, sweep_schedule=[4], rmax_schedule=[4])
    rq = O.dot(x, O.apply(A, x)) / O.dot(x, x)
    assert E[-1] > 0 and math.isclose(rq, E[-1], rel_tol=0.1)
    E, _, _ = ER.mals_eigsolve(_spd(d, 2.0), x0, sweep_schedule=[4], rmax_schedule=[4])
    assert E[-1] <= E[0] + 1e-8                              # :110-118
    x1 = O.rand_tt((2,) * d, [1] * 5, rng)
    E, x, r = ER.mals_eigsolve(_spd(d, 2.0), x1, sweep_schedule=[2, 4], rmax_schedule=[2, 4])
    assert len(E) >= 2 and max(x.ttv_rks) <= 4
    E, x, r = ER.mals_eigsolve(_spd(d, 1.0), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert all(v > 0 for v in r) and all(np.isfinite(E))
    E, x, _ = ER.mals_eigsolve(_spd(d, 2.0), x0, sweep_schedule=[2], rmax_schedule=[4], it_solver=True, itslv_thresh=1)
    assert np.isfinite(E[-1])


def test_free_fermion_formula():
    for d in (6, 8, 10):
        H = _dense_xyz(d, 0.0, 0.0, 1.0, 1.5, X)
        assert abs(ER.free_fermion_ground_energy(d, 1.0, 1.5) - np.linalg.eigvalsh(H)[0]) <= 1e-12


def test_refusals_before_the_device(T):
    """Refused in the host layer, before any handle is created: N = 1, bad schedules, a start rank beyond the SVD core moves' capacity."""
    d = 4
    A = T.Delta(d)
    x0 = to_product(O.rand_tt((2,) * d, 2, np.random.default_rng(1)))
    with pytest.raises(T.TTNError):
        T.dmrg_eigsolve(A, x0, N=1)
    for fn in (T.dmrg_eigsolve, T.mals_eigsolve):
        with pytest.raises(T.TTNError):
            fn(A, x0, sweep_schedule=[2, 2], rmax_schedule=[2, 4])
        with pytest.raises(T.TTNError):
            fn(A, x0, sweep_schedule=[0], rmax_schedule=[4])
        with pytest.raises(T.TTNError):
            fn(A, x0, sweep_schedule=[2, 4], rmax_schedule=[4])
    big = to_product(O.rand_tt((2,) * 16, [1, 2, 4, 8, 16, 32, 64, 128, 129, 128, 64, 32, 16, 8, 4, 2, 1], np.random.default_rng(2)))
    with pytest.raises(T.TTNError):
        T.dmrg_eigsolve(T.Delta(16), big)
