"""NumPy reference of contract_sites (include/ttn_contract.h): a subset C of a train's sites contracted against weight vectors, the
rest kept as a train.  Two independent ways:

    contract_dense   the dense tensor of the train (np.tensordot over the bonds), then np.tensordot with every weight vector;
    contract_chain   the kept cores, with every run of contracted sites multiplied in the OTHER association order than the device uses
                     (a run in front of a kept site from the right end of the run towards its start, the run behind the last kept site
                     from its start towards the right end).

Cores are arrays (n_k, r_{k-1}, r_k); ``weights`` maps a 0-based site to its vector.  The error bound of the tests is derived, not
measured: a chain of products with inner dimensions p_i errs by at most gamma_{sum p_i} times the same chain on absolute values, so
results are compared entrywise with  bound_factor(cores) * eps * S,  S the same contraction of |X_k| with |w_k|; the factor 2 in
bound_factor covers the reference's own rounding."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def kept_and_start(N, contracted):
    """(kept, start): the kept sites in order, and for each the first site of the run of contracted sites in front of it."""
    gone = set(contracted)
    kept, start, run = [], [], 0
    for k in range(N):
        if k not in gone:
            kept.append(k)
            start.append(run)
            run = k + 1
    return kept, start


def dense(cores):
    """the tensor of a train with end ranks 1, shape (n_1, .., n_d)"""
    t = np.asarray(cores[0])[:, 0, :]                      # (n_1, r_1)
    for c in cores[1:]:
        t = np.tensordot(t, np.asarray(c), axes=([t.ndim - 1], [1]))       # (.., n_k, r_k)
    return t[..., 0]


def contract_dense(cores, weights):
    """the dense tensor of the kept sites"""
    t = dense(cores)
    for k in sorted(weights, reverse=True):
        t = np.tensordot(t, np.asarray(weights[k], dtype=np.float64), axes=([k], [0]))
    return t


def contract_chain(cores, weights):
    """the cores of the result, (n_k, left, right) each"""
    N = len(cores)
    kept, start = kept_and_start(N, weights.keys())
    M = {k: np.tensordot(np.asarray(weights[k], dtype=np.float64), np.asarray(cores[k]), axes=([0], [0])) for k in weights}
    out = []
    for m, k in enumerate(kept):
        Y = np.array(cores[k], dtype=np.float64)
        for i in range(k - 1, start[m] - 1, -1):           # M_s (M_{s+1} (.. (M_{k-1} X[z])))
            Y = np.stack([M[i] @ Y[z] for z in range(Y.shape[0])])
        if m == len(kept) - 1:
            for i in range(k + 1, N):                      # ((X[z] M_{k+1}) M_{k+2}) ..
                Y = np.stack([Y[z] @ M[i] for z in range(Y.shape[0])])
        out.append(Y)
    return out


def abs_inputs(cores, weights):
    return [np.abs(c) for c in cores], {k: np.abs(np.asarray(v, dtype=np.float64)) for k, v in weights.items()}


def bound_factor(cores):
    """2 * sum_k (r_{k-1} + n_k): multiply by eps and by the absolute-value contraction S"""
    return 2.0 * sum(c.shape[1] + c.shape[0] for c in cores)


def site_to_grid(t, n_dims, bits, ordering):
    """The array over (2,) * (n_dims * bits) site indices as the array over grid indices, shape (2^bits,) * n_dims: the bit of level l
    (0 = most significant) of dimension m stands at site l * n_dims + m (interleaved) or m * bits + l (serial)."""
    site = (lambda m, l: l * n_dims + m) if ordering == "interleaved" else (lambda m, l: m * bits + l)
    perm = [site(m, l) for m in range(n_dims) for l in range(bits)]
    return np.transpose(t, perm).reshape((2 ** bits,) * n_dims)
