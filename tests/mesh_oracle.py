"""Independent numpy / CPU-torch restatement of the iso-surface contract of thr3ed_atom_amd.mesh (DESIGN.md "Iso-surface
extraction"): lattice sigma from CPU F.grid_sample at the float32 lattice positions, Kuhn tetrahedra enumerated from
itertools.permutations, triangle orientation from INTEGER determinants of the tet's corner offsets (the library decides it
from permutation parities), normals by autograd of grid_sample with respect to the points."""
import itertools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import relu_field_oracle as orc  # noqa: E402

C0 = 0.28209479177387814
TETS = [tuple(p) for p in itertools.permutations(range(3))]  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def tet_corners(perm):
    """the four vertices of Kuhn tet `perm` as integer offsets [4, 3]"""
    e = np.eye(3, dtype=np.int64)
    return np.stack([np.zeros(3, np.int64), e[perm[0]], e[perm[0]] + e[perm[1]], np.ones(3, np.int64)])


def lattice_coords(aabb, dims, m):
    """per axis the float32 lattice positions, guards included: R_a = m * dims[a] + 2 values"""
    out = []
    for (lo, hi), n in zip(aabb, dims):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        ext = np.float32(hi32 - lo32)
        i = np.arange(-1, m * n + 1)
        frac = (2 * i + 1).astype(np.float32) / np.float32(2 * m * n)
        c = (lo32 + ext * frac).astype(np.float32)
        c[0], c[-1] = lo32, hi32
        out.append(c)
    return out


def lattice_points(coords):
    X, Y, Z = np.meshgrid(*coords, indexing="ij")
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3)


def pre_activated(densities, density_scale, mode):
    pre = densities * density_scale
    return torch.abs(pre) if mode == "abs" else pre


def lattice_sigma(densities, aabb, density_scale, mode, m):
    """sigma on the whole lattice [Rx, Ry, Rz]: grid_sample of pre(D * rho), then post; 0 on guards / on or outside the AABB"""
    dims = tuple(densities.shape[:3])
    coords = lattice_coords(aabb, dims, m)
    pts = torch.from_numpy(lattice_points(coords))
    q = orc.normalise_points(pts, aabb)
    sigma = orc.density_activation(orc.trilinear_aten(pre_activated(densities, density_scale, mode), q), mode)[:, 0]
    sigma = torch.where(orc.inside_aabb(pts, aabb), sigma, torch.zeros_like(sigma))
    R = [len(c) for c in coords]
    sig = sigma.numpy().reshape(R).copy()
    sig[0], sig[-1], sig[:, 0], sig[:, -1], sig[:, :, 0], sig[:, :, -1] = 0, 0, 0, 0, 0, 0
    return sig, coords


def _lin(u, R):
    return (u[..., 0] * R[1] + u[..., 1]) * R[2] + u[..., 2]


def triangulate(sigma, coords, tau):
    """(edge keys [V] ascending, positions [V,3] f32, faces [T,3] int64) of {sigma > tau} on the lattice"""
    tau = np.float32(tau)
    R = np.array(sigma.shape)
    inside = sigma > tau
    keys, pos = [], []
    for code in range(1, 8):
        d = np.array([code >> 2, (code >> 1) & 1, code & 1])
        sa = sigma[: R[0] - d[0], : R[1] - d[1], : R[2] - d[2]]
        sb = sigma[d[0]:, d[1]:, d[2]:]
        cross = (sa > tau) != (sb > tau)
        u = np.argwhere(cross)
        if not len(u):
            continue
        a, b = sa[cross].astype(np.float32), sb[cross].astype(np.float32)
        t = ((tau - a) / (b - a)).astype(np.float32)
        p = np.empty((len(u), 3), np.float32)
        for ax in range(3):
            pa = coords[ax][u[:, ax]]
            diff = (coords[ax][u[:, ax] + 1] - pa).astype(np.float32) if d[ax] else np.zeros_like(pa)
            p[:, ax] = pa + (t * diff).astype(np.float32)
        keys.append(7 * _lin(u, R) + (code - 1))
        pos.append(p)
    if not keys:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    keys = np.concatenate(keys)
    pos = np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    keys, pos = keys[order], pos[order]

    Rc = tuple(int(r) - 1 for r in R)  # cubes per axis
    corner_in = {}
    for c in itertools.product((0, 1), repeat=3):
        corner_in[c] = inside[c[0]: R[0] - 1 + c[0], c[1]: R[1] - 1 + c[1], c[2]: R[2] - 1 + c[2]].reshape(-1)
    fkeys, fedges = [], []
    for ti, perm in enumerate(TETS):
        V = tet_corners(perm)
        mask = sum(corner_in[tuple(v)].astype(np.int8) << k for k, v in enumerate(V))
        for case in range(1, 15):
            sel = np.nonzero(mask == case)[0]
            if not len(sel):
                continue
            cube = np.stack(np.unravel_index(sel, Rc), axis=1)
            ins = [k for k in range(4) if (case >> k) & 1]
            out = [k for k in range(4) if not (case >> k) & 1]
            if len(ins) == 2:
                a0, a1 = ins
                b0, b1 = out
                tris = [[(a0, b0), (a0, b1), (a1, b1)], [(a0, b0), (a1, b1), (a1, b0)]]
                # outward (from the inside pair to the outside pair) iff det[a1 - a0, b0 - a0, b1 - a0] > 0
                outward = np.linalg.det(np.stack([V[a1] - V[a0], V[b0] - V[a0], V[b1] - V[a0]]).astype(float)) > 0
            else:
                s = ins[0] if len(ins) == 1 else out[0]
                o = [k for k in range(4) if k != s]
                tris = [[(s, o[0]), (s, o[1]), (s, o[2])]]
                away = np.linalg.det(np.stack([V[o[0]] - V[s], V[o[1]] - V[s], V[o[2]] - V[s]]).astype(float)) > 0
                outward = away == (len(ins) == 1)  # pointing away from s is outward when s is the inside one
            for tri_i, tri in enumerate(tris):
                if not outward:
                    tri = [tri[0], tri[2], tri[1]]
                ek = []
                for k, l in tri:
                    k, l = min(k, l), max(k, l)
                    lower = cube + V[k]
                    d = V[l] - V[k]
                    ek.append(7 * _lin(lower, R) + (4 * d[0] + 2 * d[1] + d[2] - 1))
                fedges.append(np.stack(ek, axis=1))
                fkeys.append(_lin(cube, R) * 12 + ti * 2 + tri_i)
    if not fkeys:
        return keys, pos, np.zeros((0, 3), np.int64)
    fkeys = np.concatenate(fkeys)
    fedges = np.concatenate(fedges)[np.argsort(fkeys, kind="stable")]
    faces = np.searchsorted(keys, fedges)
    assert (keys[faces] == fedges).all(), "a face references an edge without a vertex"
    return keys, pos, faces


def attributes(densities, features, aabb, density_scale, mode, positions):
    """(colours [V,3], normals [V,3], |grad| [V]) at the vertex positions"""
    K = features.shape[-1] // 3
    pts = torch.from_numpy(np.ascontiguousarray(positions)).requires_grad_(True)
    q = orc.normalise_points(pts, aabb)
    raw = orc.trilinear_aten(features[..., [0, K, 2 * K]].contiguous(), q.detach())
    colours = torch.sigmoid(raw * np.float32(C0))
    dens = orc.trilinear_aten(pre_activated(densities, density_scale, mode), q)[:, 0]
    (grad,) = torch.autograd.grad(dens.sum(), pts)
    norm = grad.norm(dim=1, keepdim=True)
    normals = torch.where(norm > 0, -grad / norm.clamp_min(1e-30), torch.zeros_like(grad))
    return colours.detach().numpy(), normals.numpy(), norm[:, 0].numpy()


def extract(densities, features, aabb, density_scale, mode, tau, m):
    """the whole contract on CPU tensors: dict(keys, vertices, faces, colours, normals, grad_norm, sigma)"""
    sigma, coords = lattice_sigma(densities, aabb, density_scale, mode, m)
    keys, pos, faces = triangulate(sigma, coords, tau)
    col, nrm, gn = attributes(densities, features, aabb, density_scale, mode, pos)
    return dict(keys=keys, vertices=pos, faces=faces, colours=col, normals=nrm, grad_norm=gn, sigma=sigma)


def manifold_report(faces, num_vertices):
    """(every undirected edge in exactly two faces, every directed edge once, Euler characteristic V - E + F)"""
    f = np.asarray(faces, np.int64)
    if not len(f):
        return True, True, 0
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = np.int64(num_vertices)
    dkey = directed[:, 0] * n + directed[:, 1]
    ukey = np.minimum(directed[:, 0], directed[:, 1]) * n + np.maximum(directed[:, 0], directed[:, 1])
    _, ucount = np.unique(ukey, return_counts=True)
    _, dcount = np.unique(dkey, return_counts=True)
    used = len(np.unique(f))
    return bool((ucount == 2).all()), bool((dcount == 1).all()), int(used - len(ucount) + len(f))
