"""NumPy restatement of the sampling semantics of include/ttn_sample.h, statement for statement, with its own splitmix64 uniforms.
Nothing here imports the package under test.

A train is a list of d cores A_k of shape (n_k, r_{k-1}, r_k).  Indices are 1-based in every output, as in the header.

    envs(cores, born)        the right environments of every bond, G_{d+1} = [1] first in the recurrence
    sample(cores, u, born)   the conditional sweep for the S rows of u: (idx, logp, margin, clamps, dead)
    evaluate(cores, idx)     x(z) at the rows of a 1-based index matrix
    dense(cores)             the full tensor (d <= 12)
    uniforms(seed, b, S, d)  the numbers the device generates for train b when no u is given
    case(name)               the named trains the CPU and the GPU tests share

margin[s] is the minimum over the sites and the INTERIOR edges c_0 .. c_{n-2} of |t - c_z| / tot: how far the draw of sample s stayed
from every decision boundary.  A sample with margin < FRAGILE is fragile: an implementation that sums in another order may draw
another index there, so exact comparisons leave it out.
"""
import numpy as np

FRAGILE = 1.0e-9
FRAGILE_SHARE = 1.0e-3          # at most 0.1 % of a case's samples may be fragile
DRAW_SAMPLE = 6
_M64 = (1 << 64) - 1


# ---- uniforms ---------------------------------------------------------------------------------------------------------------------
def subseed(seed, kind, a=0, b=0):
    p = 1000003
    return (((int(seed) * p + kind) * p + a) * p + b) & _M64


def splitmix64_word(sub, j):
    """word j (1-based) of the stream of sub-seed `sub`, in Python integers"""
    z = (sub + j * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def uniforms(seed, b, S, d):
    """(S, d): u[s, k] = (word >> 11) 2^-53 of word j = 1 + k + d s of the stream of sub-seed (seed, DRAW_SAMPLE, b, 0)"""
    sub = np.uint64(subseed(seed, DRAW_SAMPLE, b, 0))
    with np.errstate(over="ignore"):
        j = np.arange(1, S * d + 1, dtype=np.uint64)
        z = sub + j * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(S, d)


# ---- the semantics ----------------------------------------------------------------------------------------------------------------
def envs(cores, born):
    """env[m], m = 0 .. d: the environment to the right of bond m — G_{m+1} of the header for the 0-based bond m.  Born: r_m x r_m
    matrices, G_k = sum_z A_k[z] G_{k+1} A_k[z]^T.  Density: vectors, g_k = sum_z A_k[z] g_{k+1}."""
    d = len(cores)
    env = [None] * (d + 1)
    env[d] = np.ones((1, 1)) if born else np.ones(1)
    for k in range(d - 1, -1, -1):
        A = cores[k]
        acc = np.zeros((A.shape[1], A.shape[1])) if born else np.zeros(A.shape[1])
        for z in range(A.shape[0]):
            acc = acc + (A[z] @ env[k + 1] @ A[z].T if born else A[z] @ env[k + 1])
        env[k] = acc
    return env


def sample(cores, u, born):
    """The sweep of the header for the S rows of u (S, d), all samples at once; every step is the header's, per sample."""
    u = np.asarray(u, dtype=np.float64)
    S, d = u.shape
    assert d == len(cores)
    env = envs(cores, born)
    idx = np.ones((S, d), dtype=np.int64)
    logp = np.zeros(S)
    margin = np.full(S, np.inf)
    clamps = 0
    dead = np.zeros(S, dtype=bool)
    V = np.ones((S, 1))                                                   # v = [1]
    with np.errstate(all="ignore"):
        for k in range(d):
            A = cores[k]
            n = A.shape[0]
            W = np.einsum("sa,zab->szb", V, A)                            # 1. w_z = v A_k[z]
            if born:                                                      # 2.
                p = np.einsum("szb,bc,szc->sz", W, env[k + 1], W)
            else:
                p = W @ env[k + 1]
            live = ~dead
            neg = (p < 0.0) & live[:, None]                               # 3.
            clamps += int(neg.sum())
            p = np.where(p < 0.0, 0.0, p)
            c = np.cumsum(p, axis=1)                                      # 4. c_z = p_0 + .. + p_z in this order
            tot = c[:, -1]
            dies = live & (~(tot > 0.0) | ~np.isfinite(tot))              # 8.
            dead |= dies
            live = ~dead
            t = u[:, k] * tot                                             # 5.
            below = t[:, None] < c
            z = np.where(below.any(axis=1), below.argmax(axis=1), n - 1)
            pz = p[np.arange(S), z]
            logp = np.where(live, logp + np.log(pz / tot), -np.inf)       # 6.
            idx[:, k] = np.where(live, z + 1, 1)
            if n > 1:
                m = np.min(np.abs(t[:, None] - c[:, :-1]), axis=1) / tot
                margin = np.where(live, np.minimum(margin, m), margin)
            w = W[np.arange(S), z]                                        # 7. v <- w_z 2^-e, 2^e the binade of max |w_z|
            mx = np.max(np.abs(w), axis=1)
            e = np.where((mx > 0.0) & np.isfinite(mx), np.frexp(mx)[1] - 1, 0)
            V = np.where(live[:, None], np.ldexp(w, -e[:, None]), 0.0)
    return idx, logp, margin, clamps, int(dead.sum())


def evaluate(cores, idx):
    """x(z) at the rows of the 1-based (P, d) index matrix"""
    idx = np.asarray(idx)
    v = np.ones((idx.shape[0], 1))
    for k, A in enumerate(cores):
        v = np.einsum("sa,sab->sb", v, A[idx[:, k] - 1])
    return v[:, 0]


def dense(cores):
    """the full tensor x[z_1, .., z_d] (0-based array indices), d <= 12"""
    assert len(cores) <= 12
    t = np.ones((1, 1))
    for A in cores:
        t = np.einsum("pa,zab->pzb", t, A).reshape(-1, A.shape[2])
    return t.reshape([A.shape[0] for A in cores])


def target_logp(cores, idx, born):
    """log p of the header's target at the rows of idx, with the normalisation from the environments: log(x(z)^2 / <x, x>) or
    log(x(z) / sum x)"""
    x = evaluate(cores, idx)
    e0 = envs(cores, born)[0]
    with np.errstate(all="ignore"):
        return np.log(x * x / e0[0, 0]) if born else np.log(x / e0[0])


# ---- trains -----------------------------------------------------------------------------------------------------------------------
def rand_train(dims, rks, rng, positive=False, unit=False):
    """Gaussian cores scaled by 1 / sqrt(r_left) (|Gaussian| for a density); unit: every core of Frobenius norm 1"""
    cores = []
    for k, n in enumerate(dims):
        A = rng.standard_normal((n, rks[k], rks[k + 1])) / np.sqrt(rks[k])
        if positive:
            A = np.abs(A)
        if unit:
            A = A / np.linalg.norm(A)
        cores.append(A)
    return cores


def qtt_ranks(d, cap):
    return [min(2 ** k, 2 ** (d - k), cap) for k in range(d + 1)]


def full_ranks(dims, cap):
    d = len(dims)
    left = [1]
    for n in dims:
        left.append(left[-1] * n)
    right = [1]
    for n in reversed(dims):
        right.append(right[-1] * n)
    right = right[::-1]
    return [int(min(left[m], right[m], cap)) for m in range(d + 1)]


CASES = ("chip_d12", "rank80_d10", "mixed_dims", "d1", "d2", "d480", "d8_born", "d4_chi2")


def case(name, born=True):
    """(dims, trains): the trains of a named case (a list; one batch).  Density trains (born=False) have |Gaussian| cores."""
    pos = not born
    rng = np.random.default_rng([sum(map(ord, name)), int(born)])
    if name == "chip_d12":            # the on-chip class: ranks 1, 2, .., 64, .., 2, 1; a ragged batch (caps 64, 13, 7)
        dims = (2,) * 12
        return dims, [rand_train(dims, qtt_ranks(12, cap), rng, pos) for cap in (64, 13, 7)]
    if name == "rank80_d10":          # a rank-80 interior between ramps inside the class: the route changes twice per sweep
        dims = (2,) * 10
        return dims, [rand_train(dims, [1, 2, 4, 8, 16, 80, 16, 8, 4, 2, 1], rng, pos)]
    if name == "mixed_dims":          # general route, odd ranks, n != 2
        dims = (3, 2, 4, 5, 2)
        return dims, [rand_train(dims, [1, 3, 5, 7, 2, 1], rng, pos)]
    if name == "d1":
        return (2,), [rand_train((2,), [1, 1], rng, pos)]
    if name == "d2":
        return (2, 2), [rand_train((2, 2), [1, 2, 1], rng, pos)]
    if name == "d480":                # the rescale of v: 480 sites, rank 2, cores of norm 1
        dims = (2,) * 480
        return dims, [rand_train(dims, [1] + [2] * 479 + [1], rng, pos, unit=True)]
    if name == "d8_born":
        dims = (2,) * 8
        return dims, [rand_train(dims, qtt_ranks(8, 8), rng, pos)]
    if name == "d4_chi2":
        dims = (2,) * 4
        return dims, [rand_train(dims, qtt_ranks(4, 4), rng, pos)]
    raise KeyError(name)


# (case, samples per train, seed of the uniforms): what tests/test_gpu_sample.py runs in BOTH modes; tests/test_cpu_sample.py asserts that
# the reference itself draws no fragile sample on any of them
GPU_RUNS = (("chip_d12", 300, 11), ("rank80_d10", 130, 12), ("mixed_dims", 200, 13), ("d1", 65, 14), ("d2", 65, 15), ("d2", 1, 16),
            ("d480", 100, 17), ("d8_born", 4096, 18), ("d4_chi2", 20000, 19))


def run(name, S, seed, born):
    """the reference on a GPU run: (dims, trains, u (B, S, d), [sample(...) per train])"""
    dims, trains = case(name, born)
    u = np.stack([uniforms(seed, b, S, len(dims)) for b in range(len(trains))])
    return dims, trains, u, [sample(t, u[b], born) for b, t in enumerate(trains)]


def clamp_train():
    """rank-1 density train with site-1 values (2, -1): every sample draws z_1 = 1 and clamps once"""
    return (2, 2, 2), [np.array([2.0, -1.0]).reshape(2, 1, 1), np.array([1.0, 3.0]).reshape(2, 1, 1), np.array([0.5, 0.25]).reshape(2, 1, 1)]


def zero_train():
    return (2, 2, 2), [np.zeros((2, 1, 2)), np.zeros((2, 2, 2)), np.zeros((2, 2, 1))]


def chi2_stat(idx, probs):
    """Pearson's statistic of the 1-based samples idx (S, d) against the cell probabilities probs (an array of shape dims)"""
    S = idx.shape[0]
    flat = np.ravel_multi_index(tuple((idx - 1).T), probs.shape)
    obs = np.bincount(flat, minlength=probs.size).astype(np.float64)
    exp = S * probs.ravel()
    return float(np.sum((obs - exp) ** 2 / exp))
