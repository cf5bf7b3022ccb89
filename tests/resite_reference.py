"""NumPy restatement of to_qtt / to_ttv (split and merge the physical indices of a tensor train), written from the algorithm.

Cores are (n, r_left, r_right) arrays, as everywhere in this project.  Digits are big-endian: the first factor of a split list, and the
earlier core of a merged group, is the MOST significant digit of the physical index.

to_qtt, one site with factors s_1 .. s_k: for every factor but the last, view the carried block C[a, x, b] (a: left bond, x: what is
left of the physical index, b: right bond) as the matrix with rows (a, coarse digit c) and columns (fine rest f, b), x = c * fine + f,
take its thin SVD, keep U as the new core (c, a, j) and carry S V' on as C[j, f, b].  What is left after the last SVD is the last core.
Rank rule: threshold == 0 keeps every singular value (min(rows, cols)); threshold > 0 keeps those above threshold * s[0] — at least one,
the library's documented deviation for an all-zero block.

to_ttv, one group: P[a, x1, m] times the next core's G[m, x2, b] summed over m gives P'[a, x1 * n2 + x2, b].
"""
import numpy as np


class Train:
    """The four fields the product's TTvector carries (enough for tests.helpers.sign_fix_compare)."""

    def __init__(self, cores, ot=None):
        self.ttv_vec = [np.asarray(c) for c in cores]
        self.N = len(self.ttv_vec)
        self.ttv_dims = tuple(int(c.shape[0]) for c in self.ttv_vec)
        self.ttv_rks = [int(c.shape[1]) for c in self.ttv_vec] + [int(self.ttv_vec[-1].shape[2])]
        self.ttv_ot = list(ot) if ot is not None else [0] * self.N


def random_train(dims, rks, seed):
    rng = np.random.default_rng(seed)
    return Train([rng.standard_normal((dims[k], rks[k], rks[k + 1])) for k in range(len(dims))])


def dense(x):
    """The full tensor, shape ttv_dims (end ranks 1), out[i_1, ..., i_N] by plain contraction."""
    acc = np.ones((1, 1))                                        # (entries so far, bond)
    for c in x.ttv_vec:
        c = np.asarray(c)
        acc = np.einsum("pa,nab->pnb", acc, c).reshape(-1, c.shape[2])
    assert acc.shape[1] == 1
    return acc[:, 0].reshape(x.ttv_dims)


def split_site(core, factors, threshold=0.0):
    """The cores that replace `core` (n, r_l, r_r) when its physical index is split into `factors`."""
    n, rl, rr = core.shape
    assert int(np.prod(factors)) == n
    carry = np.transpose(core, (1, 0, 2))                        # C[a, x, b]
    out = []
    rest = n
    for s in factors[:-1]:
        rest //= s
        a = carry.shape[0]
        m = carry.reshape(a, s, rest, rr)                        # x = c * rest + f: C-order split of the middle axis
        m = np.transpose(m, (1, 0, 2, 3)).reshape(s * a, rest * rr)      # row c * r_prev + a: the (a + r_prev c) order
        u, sv, vt = np.linalg.svd(m, full_matrices=False)
        keep = len(sv)
        if threshold > 0.0:
            keep = max(1, int(np.count_nonzero(sv > threshold * sv[0])))
        u, sv, vt = u[:, :keep], sv[:keep], vt[:keep]
        out.append(u.reshape(s, a, keep))                        # (c, a, j)
        carry = (sv[:, None] * vt).reshape(keep, rest, rr)       # columns (f, b) in C order
    out.append(np.transpose(carry, (1, 0, 2)))
    return out


def to_qtt(x, split_dims, threshold=0.0):
    assert len(split_dims) == x.N
    cores = []
    for core, factors in zip(x.ttv_vec, split_dims):
        # the left bond of a site's first SVD is the bond the previous site ended with: unchanged by the split
        cores.extend(split_site(np.asarray(core), [int(f) for f in factors], threshold))
    return Train(cores)


def to_ttv(x, merge_numbers):
    assert sum(merge_numbers) == x.N
    cores, k = [], 0
    for count in merge_numbers:
        acc = np.asarray(x.ttv_vec[k])                           # (x1, a, m)
        for j in range(k + 1, k + count):
            g = np.asarray(x.ttv_vec[j])                         # (x2, m, b)
            acc = np.einsum("pam,qmb->pqab", acc, g).reshape(acc.shape[0] * g.shape[0], acc.shape[1], g.shape[2])
        cores.append(acc)
        k += count
    return Train(cores)
