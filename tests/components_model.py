"""numpy model of rf_label_components (include/relu_field.h) and of floater removal, written from the definitions alone and
independent of the package.

``occupied``: node n is occupied iff post(pre(D_n * rho)) > threshold, in the kernel's float32 form: the product is one float32
multiply, |.| / max(., 0) / identity are exact, and softplus is evaluated in float32 like the kernel's log1pf(expf(.)) (the tests
keep softplus thresholds away from every node's value, so its last bit cannot decide a node).
``label``: union-find over the lattice, canonicalised to the smallest plain linear index (x Y + y) Z + z of the component; -1 off it.
``sizes_of``: sizes[r] = node count of the component labelled r, 0 elsewhere.
``ranked`` / ``kept``: the order (size descending, ties by root ascending) and the keep rule (size >= min_nodes and rank < keep_largest).
``remove``: the raw densities after removal: min(D, fill) on the nodes of removed components (0 under |.|), every other bit kept."""
import numpy as np

MAX_L1 = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    """every neighbour offset of the connectivity"""
    d = MAX_L1[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 1 <= abs(dx) + abs(dy) + abs(dz) <= d]


def forward_offsets(connectivity):
    return [o for o in offsets(connectivity) if o > (0, 0, 0)]


def activated(densities, rho, mode):
    pre = np.asarray(densities, dtype=np.float32) * np.float32(rho)
    if mode == "abs":
        return np.abs(pre)
    if mode == "relu":
        return np.maximum(pre, np.float32(0.0))
    if mode == "softplus":
        with np.errstate(over="ignore"):
            return np.where(pre > np.float32(20.0), pre, np.log1p(np.exp(pre, dtype=np.float32), dtype=np.float32))
    assert mode == "identity", mode
    return pre


def occupied(densities, rho, mode, threshold):
    """densities [X,Y,Z] or [X,Y,Z,1] -> bool [X,Y,Z]"""
    d = np.asarray(densities)
    d = d[..., 0] if d.ndim == 4 else d
    return activated(d, rho, mode) > np.float32(threshold)


def label(mask, connectivity):
    """bool [X,Y,Z] -> int32 [X,Y,Z]: -1, or the smallest plain linear index of the node's component"""
    mask = np.asarray(mask, dtype=bool)
    X, Y, Z = mask.shape
    parent = np.arange(mask.size, dtype=np.int64)

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    for dx, dy, dz in forward_offsets(connectivity):
        def window(d, n):  # index ranges of the nodes that have the neighbour at +d, and of those neighbours
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (ax, bx), (ay, by), (az, bz) = window(dx, X), window(dy, Y), window(dz, Z)
        both = mask[ax, ay, az] & mask[bx, by, bz]
        for a, b in zip(idx[ax, ay, az][both], idx[bx, by, bz][both]):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)  # the smaller index stays the root: roots are canonical
    out = np.full(mask.size, -1, dtype=np.int32)
    for n in np.flatnonzero(mask.reshape(-1)):
        out[n] = find(n)
    return out.reshape(mask.shape)


def sizes_of(labels):
    flat = np.asarray(labels).reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int32)


def ranked(labels):
    """(roots, sizes) as int64 arrays: size descending, ties by root ascending"""
    sizes = sizes_of(labels).astype(np.int64)
    roots = np.flatnonzero(sizes)
    order = sorted(range(roots.size), key=lambda i: (-sizes[roots[i]], roots[i]))
    roots = roots[order] if roots.size else roots
    return roots.astype(np.int64), sizes[roots]


def kept(sizes_ranked, min_nodes=None, keep_largest=None):
    return np.array([(min_nodes is None or s >= min_nodes) and (keep_largest is None or rank < keep_largest) for rank, s in enumerate(sizes_ranked)], dtype=bool)


def remove(densities, labels, mode, min_nodes=None, keep_largest=None, fill=0.0):
    """(densities after removal -- same shape and dtype --, (components, removed_components, kept_nodes, removed_nodes))"""
    roots, sizes = ranked(labels)
    keep = kept(sizes, min_nodes, keep_largest)
    gone = np.isin(np.asarray(labels), roots[~keep])
    d = np.array(densities, dtype=np.float32, copy=True)
    view = d[..., 0] if d.ndim == 4 else d
    view[gone] = np.float32(0.0) if mode == "abs" else np.minimum(view[gone], np.float32(fill))
    return d, (int(roots.size), int((~keep).sum()), int(sizes[keep].sum()), int(sizes[~keep].sum()))


def cells_mixing_kept_and_removed(labels, keep_roots):
    """the number of cells (8 adjacent nodes) that have a corner in a kept component AND a corner in a removed one"""
    labels = np.asarray(labels)
    occ = labels >= 0
    is_kept = occ & np.isin(labels, keep_roots)
    is_gone = occ & ~is_kept
    X, Y, Z = labels.shape
    if min(X, Y, Z) < 2:
        return 0
    any_kept = np.zeros((X - 1, Y - 1, Z - 1), dtype=bool)
    any_gone = np.zeros_like(any_kept)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                any_kept |= is_kept[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]
                any_gone |= is_gone[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]
    return int((any_kept & any_gone).sum())
