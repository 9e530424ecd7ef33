"""Shared helpers of the brick-pass tests (not a test module): crafted record lists in (brick, flags) key order as the source ranks of a
data-parallel step would send them, and the float64 numpy model of what rf_brick_accumulate* must compute from them -- written from the
contract in include/relu_field.h and tied to the oracle by tests/test_brick_lists_model.py.

Records (float32 rows): full-width [n, 12] = (index x, y, z, dL/d density) (dL/d raw r, g, b, v_x) (v_y, v_z, 0, 0); base-channel
[n, 8] = (index x, y, z, 0) (dL/d density, dL/d sh0 r, g, b).  On a degree-0 grid (K = 1) every list has the base-channel format.
Channel order of the sums [X, Y, Z, 3K + 1]: 0 = density, 1..3 = degree 0 of r, g, b, 4 + (K - 1) * colour + k - 1 = degree k >= 1.

The bound of ``scatter`` is DERIVED, not measured: an element is a float32 fma chain over the ``count`` records that reach it, of
terms w_i * g_i * Y_k(v_i).  Whatever the order, the forward error of such a chain is at most (count - 1 + r) * 2^-24 * A to first
order, A = sum_i w_i |g_i| Yhat_k(v_i), where r counts the roundings inside one term (the three weights -- 1 - frac rounds in the
first cell of an axis only --, the two products between them, up to six for a basis polynomial -- Yhat_k takes every monomial in
absolute value, which covers cancellation inside the float32 evaluation --, one for g * Y: twelve at the very most) and the additions
that merge partial sums (the separable base-channel accumulators of the 4 x 8 x 8 pass: one; rf_brick_accumulate_adam_split: up to
seven, on grids of SH degree <= 2).  The bound grants r = 16: (count + 16) * 2^-24 * A."""
import itertools

import numpy as np
import torch

from oracle import relu_field_oracle as orc

U32 = 2.0 ** -24  # unit roundoff of float32
ROUNDINGS = 16
MAX_COUNT = 1600  # (MAX_COUNT + ROUNDINGS) * U32 < 1e-4: see test_brick_lists_model.py
BRICK_4X8X8 = 488


def edges_of(brick_size):
    return (4, 8, 8) if int(brick_size) == BRICK_4X8X8 else (int(brick_size),) * 3


def brick_counts(dims, edges):
    return tuple((d + e - 1) // e for d, e in zip(dims, edges))


def num_keys(dims, edges):
    nb = brick_counts(dims, edges)
    return 8 * nb[0] * nb[1] * nb[2]


def brick_key(lower, dims, edges):
    """key of include/relu_field.h: ((((bx * 2 + f_x) * NBY + by) * NBZ + bz) << 2) | f_y | f_z << 1 with (bx, by, bz) the brick of the
    cell's lower node and f_a = the cell's upper node on axis a exists and belongs to the next brick"""
    nb = brick_counts(dims, edges)
    lower = np.asarray(lower, np.int64)
    b = [lower[:, a] // edges[a] for a in range(3)]
    f = [((lower[:, a] + 1 < dims[a]) & ((lower[:, a] + 1) // edges[a] != b[a])).astype(np.int64) for a in range(3)]
    return ((((b[0] * 2 + f[0]) * nb[1] + b[1]) * nb[2] + b[2]) << 2) | f[1] | (f[2] << 1)


def key_parts(keys, dims, edges):
    """keys -> (brick id [n] = (bx * NBY + by) * NBZ + bz, flags [n, 3])"""
    nb = brick_counts(dims, edges)
    keys = np.asarray(keys, np.int64)
    fy, fz = keys & 1, (keys >> 1) & 1
    r = keys >> 2
    bz = r % nb[2]
    r = r // nb[2]
    by = r % nb[1]
    r = r // nb[1]
    fx, bx = r & 1, r >> 1
    return (bx * nb[1] + by) * nb[2] + bz, np.stack([fx, fy, fz], axis=1)


def possible_keys(dims, edges):
    """[8 * nbricks] bool: the class can hold a record (flag f_a needs a next brick on axis a)"""
    nb = brick_counts(dims, edges)
    keys = np.arange(num_keys(dims, edges))
    brick, flags = key_parts(keys, dims, edges)
    b3 = np.stack([brick // (nb[1] * nb[2]), (brick // nb[2]) % nb[1], brick % nb[2]], axis=1)
    return np.all((flags == 0) | (b3 + 1 < np.array(nb)), axis=1) & (b3[:, 0] < nb[0])


def touched_bricks(keys, dims, edges):
    """[n, 8] the ids of the bricks the records of a class touch: source + o for every offset o <= flags (-1 where there is none)"""
    nb = brick_counts(dims, edges)
    brick, flags = key_parts(keys, dims, edges)
    b3 = np.stack([brick // (nb[1] * nb[2]), (brick // nb[2]) % nb[1], brick % nb[2]], axis=1)
    out = np.full((len(brick), 8), -1, np.int64)
    for j, o in enumerate(itertools.product((0, 1), repeat=3)):
        o = np.array(o)
        ok = np.all(o <= flags, axis=1) & np.all(b3 + o < np.array(nb), axis=1)
        t = b3 + o
        out[ok, j] = ((t[:, 0] * nb[1] + t[:, 1]) * nb[2] + t[:, 2])[ok]
    return out


def keys_touching(first_brick, num_bricks, dims, edges):
    """[8 * nbricks] bool: the classes whose records touch a node of the bricks [first_brick, first_brick + num_bricks)"""
    t = touched_bricks(np.arange(num_keys(dims, edges)), dims, edges)
    return np.any((t >= first_brick) & (t < first_brick + num_bricks), axis=1)


def record_keys(rec, dims, edges):
    return brick_key(np.floor(np.asarray(rec, np.float32)[:, :3]).astype(np.int64), dims, edges)


def deal(n, num_lists, seed):
    """list of every record: uneven shares (list l gets a share proportional to l + 1), and with more than one list, list
    num_lists // 2 gets nothing"""
    if num_lists == 1:
        return np.zeros(n, np.int64)
    share = np.arange(1, num_lists + 1, dtype=np.float64)
    share[num_lists // 2] = 0.0
    return np.random.default_rng(seed).choice(num_lists, size=n, p=share / share.sum())


def sorted_lists(records, dims, edges, num_lists=1, base=0, poison=None, seed=0, tail=3):
    """Deal float32 records [n, 8 or 12] out to ``num_lists`` lists (``deal``), each in key order (stable: the record order inside a class
    is the input order) with its own offsets table: [(records [base + n_l + tail, width], int64 offsets [8 * nbricks + 1]), ...].
    ``base`` slots in front of key 0 (offsets[0] = base) and ``tail`` slots behind offsets[-1] hold NaN records -- position and values
    --, and so does every slot of a class k with poison[k] true ([8 * nbricks] bool: classes the pass must not read).  Every poisoned
    slot lies inside the array returned: the offsets never lead outside it."""
    records = np.asarray(records, np.float32)
    nkeys = num_keys(dims, edges)
    keys = record_keys(records, dims, edges)
    owner = deal(len(records), num_lists, seed)
    out = []
    for l in range(num_lists):
        mine = np.flatnonzero(owner == l)
        order = mine[np.argsort(keys[mine], kind="stable")]
        k = keys[order]
        offsets = base + np.searchsorted(k, np.arange(nkeys + 1)).astype(np.int64)
        body = records[order].copy()
        if poison is not None:
            body[np.asarray(poison, bool)[k]] = np.nan
        rec = np.full((base + len(order) + tail, records.shape[1]), np.nan, np.float32)
        rec[base: base + len(order)] = body
        assert offsets[0] == base and offsets[-1] == base + len(order) and offsets[-1] + tail == len(rec)
        out.append((rec, offsets))
    return out


def to_device(lists, diffuse, device):
    """sorted_lists output -> the (records, offsets, render_diffuse) triples of ops.brick_accumulate*_raw"""
    return [(torch.from_numpy(r).to(device), torch.from_numpy(o).to(device), bool(diffuse)) for r, o in lists]


def class_counts(lists):
    """[num_lists, 8 * nbricks] records per class, from the offsets tables alone"""
    return np.stack([np.diff(o) for _, o in lists])


# ---- channel values -------------------------------------------------------------------------------------------------------------
def _monomials(degree):
    return [(a, b, degree - a - b) for a in range(degree, -1, -1) for b in range(degree - a, -1, -1)]


def _basis_monomial_coefficients(K):
    """The oracle's basis as polynomials: coefficient of every monomial x^a y^b z^c in Y_k, read off the oracle's sh_basis by solving
    for them at random points (Y_k of band l is homogeneous of degree l) -- no constants of our own."""
    degree = int(round(np.sqrt(K))) - 1
    rng = np.random.default_rng(1)
    pts = rng.uniform(-1.0, 1.0, size=(64, 3))
    Y = orc.sh_basis(degree, torch.from_numpy(pts)).numpy()
    out = []
    for k in range(K):
        l = int(np.floor(np.sqrt(k)))
        mono = _monomials(l)
        M = np.stack([pts[:, 0] ** a * pts[:, 1] ** b * pts[:, 2] ** c for a, b, c in mono], axis=1)
        coef, *_ = np.linalg.lstsq(M, Y[:, k], rcond=None)
        assert np.abs(M @ coef - Y[:, k]).max() < 1e-12
        coef[np.abs(coef) < 1e-12] = 0.0
        out.append((mono, coef))
    return out


def sh_basis(v, K):
    """[n, K] float64 basis values of the oracle (degrees 0 to 3)"""
    degree = int(round(np.sqrt(K))) - 1
    return orc.sh_basis(degree, torch.from_numpy(np.asarray(v, np.float64))).numpy()


def sh_basis_abs(v, K):
    """Yhat_k: Y_k with every monomial taken in absolute value (>= |Y_k|)"""
    v = np.abs(np.asarray(v, np.float64))
    cols = []
    for mono, coef in _basis_monomial_coefficients(K):
        cols.append(sum(abs(c) * v[:, 0] ** a * v[:, 1] ** b * v[:, 2] ** e for (a, b, e), c in zip(mono, coef)))
    return np.stack(cols, axis=1)


def _expand(rec, wide, K, basis, mag):
    rec = np.asarray(rec, np.float32).astype(np.float64)
    C = 3 * K + 1
    out = np.zeros((len(rec), C))
    if not wide or K == 1:
        out[:, 0:4] = mag(rec[:, 4:8])
        return out
    Y = basis(rec[:, 7:10], K)
    out[:, 0] = mag(rec[:, 3])
    graw = mag(rec[:, 4:7])
    out[:, 1:4] = graw * Y[:, :1]
    for colour in range(3):
        out[:, 4 + (K - 1) * colour: 4 + (K - 1) * (colour + 1)] = graw[:, colour: colour + 1] * Y[:, 1:]
    return out


def channel_values(rec, wide, K):
    """[n, 3K + 1] float64 per-node channel values of the float32-rounded records (``wide``: full-width records of a K > 1 grid)"""
    return _expand(rec, wide, K, sh_basis, lambda x: x)


def channel_magnitudes(rec, wide, K):
    """|g| * Yhat_k(v): the per-record scale of the bound"""
    return _expand(rec, wide, K, sh_basis_abs, np.abs)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------
def _corners(rec, dims, window):
    """per corner d of the records' cells: (node index inside the window [n, 3], float64 weight [n], reaches-a-node mask [n])"""
    pos = np.asarray(rec, np.float32)[:, :3]
    fl = np.floor(pos)
    lo = fl.astype(np.int64)
    whi = pos.astype(np.float64) - fl  # exact: float64 arithmetic on the float32-rounded index
    wlo = (fl.astype(np.float64) + 1.0) - pos
    z0, z1 = window if window is not None else (0, dims[2])
    for d in range(8):
        dd = ((d >> 2) & 1, (d >> 1) & 1, d & 1)
        node = lo + np.array(dd)
        w = np.prod([whi[:, a] if dd[a] else wlo[:, a] for a in range(3)], axis=0)
        inside = np.all((node >= 0) & (node < np.array(dims)), axis=1) & (node[:, 2] >= z0) & (node[:, 2] < z1)
        node = node - np.array([0, 0, z0])
        yield node, w, inside


def scatter_parts(rec, wide, dims, K, window=None):
    """(sum64, A, count): the float64 trilinear scatter-add of the records' channel values onto the nodes [X, Y, Z, 3K + 1], the same sum
    of the magnitudes w * |g| * Yhat, and how many records reach each element (a record reaches all eight nodes of its cell that exist,
    zero weight or not).  ``window`` = (z0, z1): only the slabs z0 <= z < z1 (shape [X, Y, z1 - z0, C])."""
    C = 3 * K + 1
    shape = (dims[0], dims[1], dims[2] if window is None else window[1] - window[0])
    total, A, count = np.zeros(shape + (C,)), np.zeros(shape + (C,)), np.zeros(shape + (C,), np.int64)
    vals, mags = channel_values(rec, wide, K), channel_magnitudes(rec, wide, K)
    live = np.zeros(C, np.int64)
    live[: C if (wide and K > 1) else 4] = 1
    for node, w, inside in _corners(rec, dims, window):
        at = (node[inside, 0], node[inside, 1], node[inside, 2])
        np.add.at(total, at, w[inside, None] * vals[inside])
        np.add.at(A, at, w[inside, None] * mags[inside])
        np.add.at(count, at, live[None, :])
    return total, A, count


def bound_of(A, count):
    return (count + ROUNDINGS) * U32 * A


def scatter(rec, wide, dims, K, window=None):
    """(sum64, bound, count) with bound = (count + 16) * 2^-24 * A (module docstring)"""
    total, A, count = scatter_parts(rec, wide, dims, K, window)
    return total, bound_of(A, count), count


def expected(kinds, wide, narrow, dims, K, window=None):
    """(sum64, bound, count) of one pass over the lists of ``kinds`` (a subset of ("wide", "narrow")): the kinds share the accumulators,
    so the counts and the magnitudes add up before the bound is formed"""
    C = 3 * K + 1
    shape = (dims[0], dims[1], dims[2] if window is None else window[1] - window[0], C)
    total, A, count = np.zeros(shape), np.zeros(shape), np.zeros(shape, np.int64)
    for kind, rec in (("wide", wide), ("narrow", narrow)):
        if kind in kinds:
            t, a, c = scatter_parts(rec, kind == "wide", dims, K, window)
            total, A, count = total + t, A + a, count + c
    return total, bound_of(A, count), count


def scatter_float32(rec, wide, dims, K):
    """The same sum re-enacted in float32, one record after the other in the order given (weights, values, products and the running
    sums all rounded to float32)"""
    C = 3 * K + 1
    total = np.zeros(tuple(dims) + (C,), np.float32)
    vals = channel_values(rec, wide, K).astype(np.float32)
    nodes, terms = [], []
    for node, w, inside in _corners(rec, dims, None):
        nodes.append(np.where(inside[:, None], node, -1))
        terms.append(w.astype(np.float32)[:, None] * vals)
    nodes, terms = np.stack(nodes, axis=1).reshape(-1, 3), np.stack(terms, axis=1).reshape(-1, C)  # record-major
    ok = nodes[:, 0] >= 0
    np.add.at(total, (nodes[ok, 0], nodes[ok, 1], nodes[ok, 2]), terms[ok])
    return total


def mismatch(got, sum64, bound):
    """Largest |got - sum64| / bound over the elements (inf where an element is not finite, or differs where the bound is zero); the one
    comparison every brick-pass test goes through: a result passes when this is <= 1."""
    got = np.asarray(got, np.float64)
    assert got.shape == sum64.shape == bound.shape, (got.shape, sum64.shape, bound.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - sum64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def assert_within_bound(got, sum64, bound, what=""):
    worst = mismatch(got, sum64, bound)
    assert worst <= 1.0, f"{what}: |got - sum64| = {worst:.3g} x bound"
    return worst


def to_reference(g, K):
    """[..., 3K + 1] in channel order -> (densities [..., 1], features [..., 3K], index = colour * K + k)"""
    feat = np.zeros(g.shape[:-1] + (3 * K,), g.dtype)
    for colour in range(3):
        feat[..., colour * K] = g[..., 1 + colour]
        feat[..., colour * K + 1: colour * K + K] = g[..., 4 + (K - 1) * colour: 4 + (K - 1) * (colour + 1)]
    return g[..., :1], feat


def from_reference(dens, feat, K):
    """the inverse of ``to_reference``"""
    g = np.zeros(dens.shape[:-1] + (3 * K + 1,), dens.dtype)
    g[..., 0] = dens[..., 0]
    for colour in range(3):
        g[..., 1 + colour] = feat[..., colour * K]
        g[..., 4 + (K - 1) * colour: 4 + (K - 1) * (colour + 1)] = feat[..., colour * K + 1: colour * K + K]
    return g


def base_records(wide):
    """full-width records [n, 12] -> the base-channel format [n, 8] a degree-0 grid takes (same positions and gradients)"""
    out = np.zeros((len(wide), 8), np.float32)
    out[:, :3] = wide[:, :3]
    out[:, 4:8] = wide[:, 3:7]
    return out


# ---- crafted records ------------------------------------------------------------------------------------------------------------
def brick_of_id(brick, dims, edges):
    nb = brick_counts(dims, edges)
    return (brick // (nb[1] * nb[2]), (brick // nb[2]) % nb[1], brick % nb[2])


def holes_of(dims, edges):
    """(empty, wide_only, narrow_only) brick ids of ``crafted_records``: the last three bricks that are neither the last one (it holds the
    last node of the grid) nor among the up to eight bricks around the upper corner of brick 0 (they sum the second crowded cell) -- or
    None where the grid has no three such bricks: then every brick is reached by both kinds."""
    nb = brick_counts(dims, edges)
    n = nb[0] * nb[1] * nb[2]
    free = [b for b in range(n - 1) if max(brick_of_id(b, dims, edges)) >= 2]
    return tuple(free[-3:]) if len(free) >= 3 else None


def reaches_brick(lower, brick, dims, edges):
    """the cell with this lower node has a node (zero weight or not) in the brick"""
    b3 = np.array(brick_of_id(brick, dims, edges))
    lo, hi = b3 * np.array(edges), (b3 + 1) * np.array(edges)
    return np.all((lower + 1 >= lo) & (lower < hi), axis=1)


def hot_cells(dims, edges):
    """lower nodes of the two crowded cells: 300 records of each kind in the first, 530 (two batches of 256, or four of 128, plus a tail)
    in the second, which sits in the upper corner of brick 0 where the grid has one, so that up to eight bricks sum it"""
    first = np.array([0, 0, 0])
    second = np.array([max(0, min(e - 1, d - 2)) for d, e in zip(dims, edges)])
    assert np.any(second >= 2), "the crowded cells must not share a node"
    return (first, 300), (second, 530)


def crafted_records(dims, edges, seed, lattice=True, random_records=None):
    """(full-width records [n, 12], base-channel records [m, 8]) built to hit the edges of the brick pass.  Of each kind: a record in
    the cell of every lower node of the lattice, the last nodes included (every brick face, edge and corner, all eight flag classes,
    cells whose upper node is outside the grid), random ones, the two ``hot_cells``, records with a fractional part of exactly 0 on
    one, two and three axes.  ``holes_of``: nothing reaches the empty brick, no base-channel record the wide-only brick and no
    full-width record the narrow-only brick."""
    rng = np.random.default_rng(seed)
    dims_a = np.array(dims)
    lat = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    if random_records is None:
        random_records = int(min(1500, 4 * len(lat)))
    holes = holes_of(dims, edges)

    def lowers():
        parts = [lat] if lattice else []
        parts.append(rng.integers(0, dims_a, size=(random_records, 3)))
        for cell, n in hot_cells(dims, edges):
            parts.append(np.tile(cell[None], (n, 1)))
        return np.concatenate(parts)

    def positions(lower):
        pos = (lower + rng.uniform(0.0, 1.0, size=lower.shape)).astype(np.float32)
        # fractional part exactly 0 on one, two and three axes, spread over the records (crowded cells and last cells included)
        for naxes, start in ((1, 0), (2, 1), (3, 2)):
            rows = np.arange(start, len(pos), 23)
            for j, r in enumerate(rows):
                axes = [(j + t) % 3 for t in range(naxes)]
                pos[r, axes] = lower[r, axes]
        # (float32 rounding must not push a position into the next cell or out of the grid)
        return np.minimum(pos, np.nextafter((lower + 1).astype(np.float32), np.float32(0.0)))

    def keep(lower, avoid):
        ok = np.ones(len(lower), bool)
        if holes is not None:
            for b in avoid:
                ok &= ~reaches_brick(lower, holes[b], dims, edges)
        return lower[ok]

    wl = keep(lowers(), (0, 2))
    nl = keep(lowers(), (0, 1))
    wide = np.zeros((len(wl), 12), np.float32)
    wide[:, :3] = positions(wl)
    wide[:, 3:7] = rng.uniform(-1.0, 1.0, size=(len(wide), 4))
    v = rng.normal(size=(len(wide), 3))
    wide[:, 7:10] = v / np.linalg.norm(v, axis=1, keepdims=True)
    narrow = np.zeros((len(nl), 8), np.float32)
    narrow[:, :3] = positions(nl)
    narrow[:, 4:8] = rng.uniform(-1.0, 1.0, size=(len(narrow), 4))
    for rec, lower in ((wide, wl), (narrow, nl)):
        assert np.array_equal(np.floor(rec[:, :3]).astype(np.int64), lower)
    return wide, narrow


def narrow_pass_records(dims, seed):
    """The record set of tests/test_hip_brick_narrow.py (4 x 8 x 8 bricks): (full-width records [n, 12], base-channel records [m, 8]).  Base-channel records: one per lower node of the lattice of every
    node (every brick face, edge and corner), more at random, 300 in one cell (several batches for one brick); full-width records
    only at lower x <= 6 and base-channel ones only at lower x >= 4 (bricks with one kind only); nothing that reaches a node with
    y >= 8 and z >= 16 (empty bricks)."""
    rng = np.random.default_rng(seed)
    X, Y, Z = dims

    def positions(lower):
        return lower + rng.uniform(0.0, 1.0, size=lower.shape).astype(np.float32)

    lat = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3)
    narrow_lower = np.concatenate([lat[lat[:, 0] >= 4], np.tile([[6, 3, 5]], (300, 1)),
                                   rng.integers(0, np.array(dims), size=(2000, 3))])
    narrow_lower = narrow_lower[narrow_lower[:, 0] >= 4]
    wide_lower = np.concatenate([lat[(lat[:, 0] <= 6) & (lat % 3 == 0).any(axis=1)], rng.integers(0, np.array(dims), size=(1500, 3))])
    wide_lower = wide_lower[wide_lower[:, 0] <= 6]
    keep = lambda lo: ~((lo[:, 1] + 1 >= 8) & (lo[:, 2] + 1 >= 16))
    narrow_lower, wide_lower = narrow_lower[keep(narrow_lower)], wide_lower[keep(wide_lower)]
    narrow = np.zeros((len(narrow_lower), 8), np.float32)
    narrow[:, :3] = positions(narrow_lower)
    narrow[:, 4:8] = rng.uniform(-1.0, 1.0, size=(len(narrow), 4))
    wide = np.zeros((len(wide_lower), 12), np.float32)
    wide[:, :3] = positions(wide_lower)
    wide[:, 3:7] = rng.uniform(-1.0, 1.0, size=(len(wide), 4))
    v = rng.normal(size=(len(wide), 3))
    wide[:, 7:10] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return wide, narrow



# ---- Adam -----------------------------------------------------------------------------------------------------------------------
def adam_reference(p0, m0, v0, g, lr, b1, b2, eps, step):
    """float64 torch.optim.Adam step -> (p, m, v)"""
    p0, m0, v0 = (np.asarray(t, np.float64) for t in (p0, m0, v0))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m = m0 + (g - m0) * (1.0 - b1)
    v = v0 * b2 + g * g * (1.0 - b2)
    p = p0 - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def assert_adam_close(p1, m1, v1, p, m, v, lr):
    """the tolerances of tests/test_hip_brick_narrow.py::test_brick_adam_with_base_channel_records"""
    np.testing.assert_allclose(m1, m, rtol=1e-5, atol=1e-5 * float(np.abs(m).max()))
    np.testing.assert_allclose(v1, v, rtol=1e-5, atol=1e-6 * float(np.abs(v).max()))
    np.testing.assert_allclose(p1, p, rtol=0, atol=1e-5 * lr + 2e-7)


# ---- the grids of tests/test_hip_brick_matrix.py (test_brick_lists_model.py holds the coverage conditions for every one of them) ----
GRIDS = (
    (10, 13, 17),  # no multiple of any brick edge
    (16, 16, 24),  # exact multiples, several bricks per axis: interior bricks have all seven lower neighbours
    (3, 5, 6),     # smaller than one 8^3 / 4 x 8 x 8 brick on every axis
    (20, 4, 19),   # one brick thick on y
)
RANGE_GRID = (20, 13, 17)  # three and more x-slabs of bricks
BRICK_SIZES = (4, 8, BRICK_4X8X8)
# more than 2^24 padded nodes, so that brick size 8 takes the optimizer flush that is not one-round.  The ABI takes at most 2046 nodes
# per axis (check_grid: RF_ERR_BAD_SHAPE above), so the grid is a thin slab rather than a long bar: 8 x 1032 x 2048 padded = 16.9 M
LONG_GRID = (8, 1026, 2046)
LONG_WINDOW = 48  # slabs per window of the long grid's host reference


def long_grid_windows(seed):
    """(z0, z1) windows of LONG_GRID that hold records: both ends and four at random, disjoint, aligned to the brick"""
    rng = np.random.default_rng(seed)
    Z = LONG_GRID[2]
    mids = sorted(int(z) for z in rng.choice(np.arange(1, Z // 128 - 1), size=4, replace=False) * 128)
    return [(0, LONG_WINDOW)] + [(z, z + LONG_WINDOW) for z in mids] + [(Z - LONG_WINDOW, Z)]


def long_grid_records(seed, per_window=1200):
    """base-channel records [n, 8] on LONG_GRID: in every window of ``long_grid_windows`` random records whose cells lie inside the
    window (the first and the last cell along z included), one crowded cell of 530 and the last cell of the grid"""
    rng = np.random.default_rng(seed)
    X, Y, Z = LONG_GRID
    lowers = []
    for z0, z1 in long_grid_windows(seed):
        top = min(z1 - 1, Z) if z1 < Z else Z  # the upper node of a cell stays inside the window (or outside the grid)
        lo = np.stack([rng.integers(0, X, per_window), rng.integers(0, Y, per_window), rng.integers(z0, top, per_window)], axis=1)
        lo[0] = (X - 1, Y - 1, top - 1)
        lo[1] = (0, 0, z0)
        lowers += [lo, np.tile([[3, 7, z0 + 7]], (530, 1))]
    lower = np.concatenate(lowers)
    rec = np.zeros((len(lower), 8), np.float32)
    pos = (lower + rng.uniform(0.0, 1.0, size=lower.shape)).astype(np.float32)
    rec[:, :3] = np.minimum(pos, np.nextafter((lower + 1).astype(np.float32), np.float32(0.0)))
    rec[:, 4:8] = rng.uniform(-1.0, 1.0, size=(len(rec), 4))
    assert np.array_equal(np.floor(rec[:, :3]).astype(np.int64), lower)
    return rec
