"""CPU-side tests (no GPU) of the excited-state scheme of csrc/ttn_eig_ortho_kernels.h through its NumPy restatement
(tests/eig_ortho_reference.py): no penalty = eig_reference.py bit for bit, levels 0..3 of three operators against the dense spectrum,
the free-fermion levels of the open Ising chain, the host-side refusals that need no device, and a source check that the kernel's
copies of the walk and of the Lanczos routine still match the plain ones."""
import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import eig_ortho_reference as EO
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def _lap(d, shift=0.5):
    return O.tto_add(O.Delta(d), O.tto_scale(shift, O.id_tto(d)))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("it_solver", [False, True])
def test_no_penalty_is_the_plain_restatement(mode, it_solver):
    d = 6
    A = _lap(d)
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(2 + mode))
    kw = dict(tol=1e-10, sweep_schedule=[2, 3], rmax_schedule=[2, 4], it_solver=it_solver, linsolv_tol=1e-10)
    E0, x0r, r0 = ER.two_site_eigsolve(mode, A, x0, **kw)
    E1, x1r, r1, ovl = EO.two_site_eigsolve_ortho(mode, A, x0, [], [], **kw)
    assert E1 == E0 and r1 == r0 and ovl == []
    assert list(x1r.ttv_rks) == list(x0r.ttv_rks) and list(x1r.ttv_ot) == list(x0r.ttv_ot)
    for a, b in zip(x1r.ttv_vec, x0r.ttv_vec):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_levels_against_dense_spectrum(T, mode, case):
    """Levels 0..3, weight 10, rank-2 random starts: |rayleigh - ev_k| <= 1e-8 and |<phi_j, x>| / ||phi_j|| <= 1e-8 for every earlier j.
    XXX at d = 6: the singlet, then the threefold triplet found one vector after another."""
    name, A, seed, kw = EO.level_cases()[case]
    ev = np.linalg.eigvalsh(O.qtto_to_matrix(A))
    E, xs = EO.lowest_states(mode, A, EO.level_starts(A, seed + mode), 4, 10.0, **kw)
    for k in range(4):
        print(name, mode, k, "energy error %.3e" % abs(E[k] - ev[k]))
        assert abs(E[k] - ev[k]) <= 1e-8, (name, k)
        for j in range(k):
            o = abs(float(O.dot(xs[j], xs[k]))) / np.sqrt(float(O.dot(xs[j], xs[j])))
            print(name, mode, k, j, "overlap %.3e" % o)
            assert o <= 1e-8, (name, k, j)
    if name == "xxx":
        assert abs(ev[1] - ev[3]) <= 1e-12 and ev[1] - ev[0] > 0.1          # the triplet above the singlet


def test_overlaps_from_the_chains():
    """The overlaps the walk returns (read from the chains) are those of the final state."""
    d = 6
    A = _lap(d)
    rng = np.random.default_rng(9)
    phis = [O.rand_tt((2,) * d, r, rng) for r in (1, 3)]
    _, x, _, ovl = EO.two_site_eigsolve_ortho(1, A, O.rand_tt((2,) * d, 2, rng), phis, [10.0, 7.0], tol=1e-10, sweep_schedule=[3],
                                              rmax_schedule=[4])
    for p, o in zip(phis, ovl):
        assert abs(o - float(O.dot(p, x)) / np.sqrt(float(O.dot(p, p)))) <= 1e-13


def test_free_fermion_levels(T):
    d = 8
    ev = np.linalg.eigvalsh(O.qtto_to_matrix(to_oracle(T.ising_tto(d, J=1.0, h=1.5))))
    E0, E1, E2 = EO.free_fermion_levels(d, 1.0, 1.5)
    assert abs(E0 - ER.free_fermion_ground_energy(d, 1.0, 1.5)) <= 1e-12
    assert abs(ev[0] - E0) <= 1e-12 and abs(ev[1] - E1) <= 1e-12 and abs(ev[2] - E2) <= 1e-12
    assert abs(ev[3] + 10.704) <= 1e-3 and abs(ev[4] + 10.1616) <= 1e-4 and abs(ev[4] - (E1 + E2 - E0)) <= 1e-12


def test_host_refusals_without_device(T):
    d = 4
    A = T.Delta(d)
    x0 = to_product(O.rand_tt((2,) * d, 2, np.random.default_rng(1)))
    phi = to_product(O.rand_tt((2,) * d, 2, np.random.default_rng(2)))
    for fn in (T.dmrg_eigsolve, T.mals_eigsolve):
        with pytest.raises(T.TTNError, match="weight without ortho_to"):
            fn(A, x0, weight=10.0)
        with pytest.raises(T.TTNError, match="needs weight"):
            fn(A, x0, ortho_to=[phi])
        with pytest.raises(T.TTNError, match="weight"):
            fn(A, x0, ortho_to=[phi], weight="heavy")
        with pytest.raises(T.TTNError, match="fits neither"):
            fn(A, x0, ortho_to=[phi, phi], weight=[1.0, 2.0, 3.0])
        with pytest.raises(T.TTNError, match="finite and > 0"):
            fn(A, x0, ortho_to=[phi], weight=-1.0)
        with pytest.raises(T.TTNError, match="at most 8"):
            fn(A, x0, ortho_to=[phi] * 9, weight=1.0)
    with pytest.raises(T.TTNError, match="N = 2"):
        T.dmrg_eigsolve(A, x0, N=3, ortho_to=[phi], weight=10.0)
    with pytest.raises(T.TTNError, match="N = 2"):
        T.lowest_states(A, x0, 2, 10.0, N=1)


def _block(text, start):
    """The brace-matched body that follows `start` in `text`, as stripped non-empty lines."""
    i = text.index("{", text.index(start))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return [ln.strip() for ln in text[i + 1:j - 1].splitlines() if ln.strip()]


def test_the_two_copies_of_the_walk_and_of_lanczos_agree():
    """csrc/ttn_eig_ortho_kernels.h carries its own copy of k_two_site_eig's walk and of wg_lanczos_smallest (so that the plain kernel
    keeps its machine code).  Nothing else keeps them in step: apart from the calls into the penalty, the statements must be the same."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensortrainnumerics.jl_amd", "csrc")
    plain = open(os.path.join(csrc, "ttn_eigsolve_kernels.h")).read()
    ortho = open(os.path.join(csrc, "ttn_eig_ortho_kernels.h")).read()
    lz_plain = _block(plain, "int wg_lanczos_smallest(")
    lz_ortho = [ln for ln in _block(ortho, "int wg_lanczos_penalised(") if ln != "extra(vj, w, N);"]
    assert len(lz_ortho) == len(lz_plain) and lz_ortho == lz_plain
    walk_plain = [ln for ln in _block(plain, "k_two_site_eig(EigArgs R)") if "wg_lanczos_smallest(" not in ln and ln != "extern __shared__ double lds[];"]
    hooks = [ln for ln in _block(ortho, "void two_site_eig_ortho_walk(") if "pen." in ln]
    walk_ortho = [ln for ln in _block(ortho, "void two_site_eig_ortho_walk(") if "pen." not in ln]
    assert walk_ortho == walk_plain
    # the calls into the penalty: begin, project, dense, the Lanczos call with its extra term, moved, finish
    assert len(hooks) == 6 and sum("wg_lanczos_penalised(" in ln for ln in hooks) == 1
