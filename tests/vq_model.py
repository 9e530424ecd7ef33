"""The numpy float64 model of vector quantisation: true squared distances, the bound E within which a float32
expansion-form ranking value lies of the true distance, the check a returned assignment has to pass, the partition of the nodes by
importance shares, the weighted centroid, a float32 restatement of the expansion form the kernel ranks by, and the four kinds of
input the bound was examined on.  Nothing here imports the code under test."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
PRUNED, KEPT, QUANTISED = 0, 1, 2
INPUT_KINDS = ("uniform", "near_codeword", "duplicated", "offset")
CENTRED_KINDS = INPUT_KINDS[:3]


def sq_distances(x, c):
    """[M, C] float64: sum_k (x_k - c_k)^2"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def bound_E(x, c):
    """[M, C] float64: E(x, c) = (D + 4) u (||x||^2 + 2 sum_k |x_k c_k| + ||c||^2)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    D = x.shape[1]
    return (D + 4) * U * ((x * x).sum(-1)[:, None] + 2.0 * np.abs(x) @ np.abs(c).T + (c * c).sum(-1)[None, :])


def assignment_excess(x, c, index, chunk=256):
    """Per row: (d(x, c_j) - min_i [d(x, c_i) + E(x, c_i)]) / E(x, c_j) for the returned j.  The assignment is consistent with every
    computed distance lying within E of the true one iff this is <= 1 (d_j - E_j <= min_i [d_i + E_i])."""
    x, c, index = np.asarray(x, np.float64), np.asarray(c, np.float64), np.asarray(index, np.int64)
    out = np.empty(x.shape[0])
    for lo in range(0, x.shape[0], chunk):
        rows = np.arange(lo, min(lo + chunk, x.shape[0]))
        d, E = sq_distances(x[rows], c), bound_E(x[rows], c)
        j = index[rows]
        pick = (np.arange(rows.size), j)
        gap = d[pick] - (d + E).min(1)
        Ej = E[pick]  # (0 only for an all-zero pair)
        out[rows] = np.where(Ej > 0.0, gap / np.where(Ej > 0.0, Ej, 1.0), np.where(gap <= 0.0, 0.0, np.inf))
    return out


def assignment_ok(x, c, index):
    return assignment_excess(x, c, index) <= 1.0


def expansion_assign_f32(x, c):
    """The form the kernel ranks by, restated in numpy: s = ||c||^2 - 2 x.c as one float32 chain in ascending k that starts from
    ||c||^2 (summed in float64, rounded once); the lowest index among equal values.  Every step is rounded to float32 from the
    float64 sum of the accumulator and the exact product."""
    x32, c32 = np.asarray(x, np.float32), np.asarray(c, np.float32)
    acc = (c32.astype(np.float64) ** 2).sum(-1).astype(np.float32)[None, :].repeat(x32.shape[0], 0)
    for k in range(x32.shape[1]):
        prod = (-2.0 * x32[:, k].astype(np.float64))[:, None] * c32[:, k].astype(np.float64)[None, :]
        acc = (acc.astype(np.float64) + prod).astype(np.float32)
    return acc.argmin(1)


def partition_by_shares(importance, prune_share, keep_share):
    """uint8 classes in node order.  Rank: more important first, lower node index first among equals.  PRUNED: the inclusive float64
    sum from the least important node up is <= prune_share x total.  KEPT: not pruned and the sum over the nodes ranked before it is
    < keep_share x total.  QUANTISED: the rest.  (Plain loops: the sums are sequential.)"""
    imp = [float(v) for v in np.asarray(importance, np.float64).reshape(-1)]
    rank = sorted(range(len(imp)), key=lambda i: (-imp[i], i))
    classes = np.full(len(imp), QUANTISED, np.uint8)
    total = 0.0
    for i in reversed(rank):
        total += imp[i]
    running = 0.0
    for i in reversed(rank):
        running += imp[i]
        if running <= prune_share * total:
            classes[i] = PRUNED
    before = 0.0
    for i in rank:
        if classes[i] != PRUNED and before < keep_share * total:
            classes[i] = KEPT
        before += imp[i]
    return classes


def weighted_centroid(x, w, members):
    """float64 sum w x / sum w over ``members`` (row indices), and sum w |x| / sum w -- the scale of the centroid's error bound"""
    x, w = np.asarray(x, np.float64)[members], np.asarray(w, np.float64)[members]
    return (w[:, None] * x).sum(0) / w.sum(), (w[:, None] * np.abs(x)).sum(0) / w.sum()


def make_inputs(kind, M, C, D, seed):
    """(x [M, D], c [C, D]) float32: U(-1, 1) data and codes; vectors 1e-4 from a codeword; a codebook whose second half repeats its
    first (code j + C // 2 is the twin of code j < C // 2); the uniform data offset by +100"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (M, D)).astype(np.float32)
    c = rng.uniform(-1.0, 1.0, (C, D)).astype(np.float32)
    if kind == "near_codeword":
        x = (c[rng.integers(0, C, M)] + rng.uniform(-1e-4, 1e-4, (M, D))).astype(np.float32)
    elif kind == "duplicated":
        half = C // 2
        c[half:2 * half] = c[:half]
    elif kind == "offset":
        x, c = x + np.float32(100.0), c + np.float32(100.0)
    elif kind != "uniform":
        raise ValueError(kind)
    return x, c
