"""Float64 numpy model of rf.MeshTextureSampler / rf.fit_texture (rf_mesh_raster_taps, rf_texture_sample and
rf_texture_sample_backward of include/relu_field.h), restated independently from the contract: the tap record
of a pixel from its barycentrics and its face's UVs, the forward from the taps, the transposed sum as one scatter over (texel, pixel,
weight) triples -- no sort, no segments, no two paths --, the loss of ``fit_texture`` and a plain Adam loop.  ``transposed`` also
returns the per-texel rounding bound of docs/texture_fit_errors.md, (n + 3) u sum |terms| with n the texel's entry count.  The inputs
the GPU test runs (``CASES`` / ``make_case``, ``crafted_list``) live here too, so that the CPU tests can show on exactly those inputs
that the comparison can fail (``WRONG``)."""
import numpy as np

from tests import mesh_raster_model as mrm
from tests.helpers import hash_uniform
from thr3ed_atom_amd.texture import atlas_layout, corner_uvs

UNIT = 2.0 ** -24  # float32 unit round-off
NO_TAP = 0xFFFF
WRONG = ("fx_fy_swapped", "duplicate_dropped", "alpha_ignored")
FORWARD_ROUNDINGS = 8  # the fetch rounds each product chain at most 6 times (docs/texture_fit_errors.md); 8 u sum |terms| bounds it


def taps_from_barycentrics(bary, face_ids, uvs, Ht, Wt):
    """bary [P, 3], face_ids [P] (-1: no hit), uvs [T, 3, 2] -> dict of x0, x1, y0, y1 int64 [P] (NO_TAP where nothing was hit) and
    fx, fy float64 [P]: texel coordinates (u Wt - 1/2, (1 - v) Ht - 1/2), the taps clamped to the texture"""
    bary, face_ids = np.asarray(bary, np.float64).reshape(-1, 3), np.asarray(face_ids, np.int64).reshape(-1)
    hit = face_ids >= 0
    uv = (bary[..., None] * np.asarray(uvs, np.float64).reshape(-1, 3, 2)[np.maximum(face_ids, 0)]).sum(1) if len(np.asarray(uvs).reshape(-1)) else np.zeros((len(bary), 2))
    x, y = uv[:, 0] * Wt - 0.5, (1.0 - uv[:, 1]) * Ht - 0.5
    xf, yf = np.floor(x), np.floor(y)
    cl = lambda a, n: np.where(hit, np.clip(a, 0, n - 1), NO_TAP).astype(np.int64)  # noqa: E731
    return dict(x0=cl(xf, Wt), x1=cl(xf + 1, Wt), y0=cl(yf, Ht), y1=cl(yf + 1, Ht), fx=np.where(hit, x - xf, 0.0), fy=np.where(hit, y - yf, 0.0))


def taps_from_records(words):
    """the device's RFTextureTap records as int32 words [P, 4] -> the dict of ``taps_from_barycentrics`` (fx, fy: the float32 values)"""
    words = np.ascontiguousarray(words, np.int32).reshape(-1, 4)
    xs, ys = words[:, 0].astype(np.int64), words[:, 1].astype(np.int64)
    frac = words[:, 2:4].copy().view(np.float32).astype(np.float64)
    return dict(x0=xs & 0xFFFF, x1=(xs >> 16) & 0xFFFF, y0=ys & 0xFFFF, y1=(ys >> 16) & 0xFFFF, fx=frac[:, 0], fy=frac[:, 1])


def hit_of(taps):
    return taps["x0"] != NO_TAP


def forward(taps, texture, background=0.0):
    """colour [P, 3]: the bilinear blend of the four taps, ``background`` where nothing was hit"""
    tex = np.asarray(texture, np.float64)
    hit = hit_of(taps)
    z = lambda a: np.where(hit, a, 0)  # noqa: E731
    x0, x1, y0, y1, fx, fy = z(taps["x0"]), z(taps["x1"]), z(taps["y0"]), z(taps["y1"]), taps["fx"][:, None], taps["fy"][:, None]
    colour = (1 - fy) * ((1 - fx) * tex[y0, x0] + fx * tex[y0, x1]) + fy * ((1 - fx) * tex[y1, x0] + fx * tex[y1, x1])
    return np.where(hit[:, None], colour, float(background))


def triples(taps, Wt, wrong=None):
    """(texel, pixel, weight) of every entry, four per hit pixel, in no particular order"""
    pixel = np.nonzero(hit_of(taps))[0]
    x0, x1, y0, y1, fx, fy = (taps[k][pixel] for k in ("x0", "x1", "y0", "y1", "fx", "fy"))
    if wrong == "fx_fy_swapped":
        fx, fy = fy, fx
    texel = np.stack([y0 * Wt + x0, y0 * Wt + x1, y1 * Wt + x0, y1 * Wt + x1], 1)
    weight = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    keep = np.ones(texel.shape, bool)
    if wrong == "duplicate_dropped":  # a tap clamped onto its neighbour is two entries on one texel: the doctored list keeps the first
        keep[:, 1] &= x1 != x0
        keep[:, 2] &= y1 != y0
        keep[:, 3] &= (x1 != x0) & (y1 != y0)
    return texel[keep], np.repeat(pixel[:, None], 4, 1)[keep], weight[keep]


def transposed(taps, grad_colour, Ht, Wt, wrong=None):
    """(grad_texture [Ht Wt, 3], bound [Ht Wt, 3], counts [Ht Wt]) of the adjoint applied to grad_colour [P, 3]"""
    texel, pixel, weight = triples(taps, Wt, wrong)
    g = np.asarray(grad_colour, np.float64).reshape(-1, 3)
    terms = weight[:, None] * g[pixel]
    grad, mag = np.zeros((Ht * Wt, 3)), np.zeros((Ht * Wt, 3))
    np.add.at(grad, texel, terms)
    np.add.at(mag, texel, np.abs(terms))
    counts = np.bincount(texel, minlength=Ht * Wt).astype(np.int64)
    return grad, segment_bound(counts, mag), counts


def segment_bound(counts, magnitudes):
    """(n + 3) u sum |terms| per texel (docs/texture_fit_errors.md)"""
    return (np.asarray(counts, np.float64)[:, None] + 3.0) * UNIT * magnitudes


def loss_and_grad(taps, texture, images, alphas, background, loss="l2", wrong=None):
    """the loss of rf.fit_texture without D-SSIM -- the mean over the hit pixels and their channels of the squared or absolute residual of
    m s + (1 - m) background -- and its gradient with respect to the sampled colours s [P, 3]"""
    hit = hit_of(taps)
    s = forward(taps, texture, background)
    m = np.ones((len(s), 1)) if alphas is None else np.asarray(alphas, np.float64).reshape(-1, 1)
    pred = m * s + (0.0 if wrong == "alpha_ignored" else (1 - m) * float(background))
    residual = np.where(hit[:, None], pred - np.asarray(images, np.float64).reshape(-1, 3), 0.0)
    terms = 3.0 * max(int(hit.sum()), 1)
    if loss == "l2":
        return (residual ** 2).sum() / terms, 2.0 * residual * m / terms
    return np.abs(residual).sum() / terms, np.sign(residual) * m / terms


def adam_fit(taps, start, images, alphas, background, iterations, lr, loss="l2", betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam on the texture, clamped to [0, 1] after each step where some pixel taps: (losses before each step, texture)"""
    Ht, Wt = np.asarray(start).shape[:2]
    texture = np.asarray(start, np.float64).copy()
    covered = (transposed(taps, np.zeros((len(taps["x0"]), 3)), Ht, Wt)[2] > 0).reshape(Ht, Wt, 1)
    m1, m2, losses = np.zeros_like(texture), np.zeros_like(texture), []
    for step in range(1, iterations + 1):
        value, gs = loss_and_grad(taps, texture, images, alphas, background, loss)
        g = transposed(taps, gs, Ht, Wt)[0].reshape(Ht, Wt, 3)
        losses.append(value)
        m1 = betas[0] * m1 + (1 - betas[0]) * g
        m2 = betas[1] * m2 + (1 - betas[1]) * g * g
        update = (lr / (1 - betas[0] ** step)) * m1 / (np.sqrt(m2) / np.sqrt(1 - betas[1] ** step) + eps)
        texture = np.where(covered, np.clip(texture - update, 0.0, 1.0), texture)
    return np.array(losses), texture


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test (tests/test_hip_texture_fit.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _views(seed, n, away=()):
    """n poses near one base pose (view 0 is the base itself); the views listed in ``away`` look the other way, past the mesh"""
    R, t = mrm.pose(seed)
    out = []
    for k in range(n):
        a = 0.06 * hash_uniform((3,), seed + 100 + k).astype(np.float64) * (k > 0)
        skew = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        q, _ = np.linalg.qr(np.eye(3) + skew)
        q = q * np.sign(np.diag(q))[None, :]
        Rk = R.astype(np.float64) @ q
        if k in away:
            Rk = Rk @ np.diag([-1.0, 1.0, -1.0])
        out.append((Rk.astype(np.float32), (t + (0.05 * hash_uniform((3,), seed + 200 + k) * (k > 0))).astype(np.float32)))
    return out


def _case(name, H, W, focal, views, tris, seed, patch=None, texture_shape=None, near=0.0, cull=False, background=0.0):
    vertices, faces = mrm.soup(tris)
    T = len(faces)
    if patch is not None:
        lay = atlas_layout(T, patch)
        uvs, shape = corner_uvs(lay, T), (lay.height, lay.width)
    else:  # a free texture: random UVs, some of them outside [0, 1] so that taps clamp
        uvs, shape = (0.5 + 0.7 * hash_uniform((T, 3, 2), seed + 60)).astype(np.float32), texture_shape
    texture = (hash_uniform(shape + (3,), seed + 50) * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    return dict(name=name, H=H, W=W, focal=float(np.float32(focal)), views=views, vertices=vertices, faces=faces, uvs=uvs, texture=texture, near=near, cull=cull,
                background=background)


def _builders():
    B = {}

    def one_face_fills_the_frame(seed):  # patch 2: every texel of the face gets thousands of entries
        H, W, f, views = 48, 64, 50.0, _views(seed, 3)
        tri = mrm.unproject([[-400.0, -300.0], [600.0, -200.0], [40.0, 800.0]], [3.0, 2.5, 3.5], H, W, f, *views[0])
        return _case("T1-P2-48x64-v3", H, W, f, views, [tri], seed, patch=2)
    B["T1-P2-48x64-v3"] = one_face_fills_the_frame

    def one_pixel(seed):
        views = _views(seed, 1)
        tris = [mrm.unproject([[-3.0, -3.0], [5.0, -2.0], [0.0, 6.0]], [2.0, 2.0, 3.0], 1, 1, 1.5, *views[0]),
                mrm.unproject([[3.0, 3.0], [5.0, 3.0], [4.0, 6.0]], [1.0, 1.0, 1.0], 1, 1, 1.5, *views[0])]
        return _case("T2-P3-1x1-v1", 1, 1, 1.5, views, tris, seed, patch=3)
    B["T2-P3-1x1-v1"] = one_pixel

    def stacked(seed):  # three large faces behind one another; the last view looks past the mesh
        H, W, f, views = 24, 40, 30.0, _views(seed, 3, away=(2,))
        return _case("T3-P8-24x40-v3", H, W, f, views, mrm.large_triangles(3, H, W, f, *views[0], seed + 5, 0.2), seed, patch=8, background=1.0)
    B["T3-P8-24x40-v3"] = stacked

    def many(seed):
        H, W, f, views = 37, 53, 45.0, _views(seed, 17, away=(5,))
        tris = np.concatenate([mrm.small_triangles(30, H, W, f, *views[0], seed + 5, 5.0), mrm.large_triangles(7, H, W, f, *views[0], seed + 9, 0.3)])
        return _case("T37-P3-37x53-v17", H, W, f, views, tris, seed, patch=3)
    B["T37-P3-37x53-v17"] = many

    def culled_and_near(seed):  # every other face runs the other way; near = 2.3 drops the faces with a corner in front of it
        H, W, f, views = 24, 40, 30.0, _views(seed, 2)
        tris = mrm.large_triangles(9, H, W, f, *views[0], seed + 5, 0.1)
        tris[::2] = tris[::2, ::-1].copy()
        return _case("T9-P2-24x40-v2-cull-near", H, W, f, views, tris, seed, patch=2, near=2.3, cull=True, background=1.0)
    B["T9-P2-24x40-v2-cull-near"] = culled_and_near

    def one_texel(seed):  # a 1 x 1 texture: every tap is clamped, x0 == x1 and y0 == y1
        H, W, f, views = 24, 40, 30.0, _views(seed, 2)
        return _case("T2-tex1x1-24x40-v2", H, W, f, views, mrm.large_triangles(2, H, W, f, *views[0], seed + 5, 0.1), seed, texture_shape=(1, 1))
    B["T2-tex1x1-24x40-v2"] = one_texel

    def free_texture(seed):  # a 5 x 7 texture with UVs that leave it: taps clamped on every edge
        H, W, f, views = 24, 40, 30.0, _views(seed, 2)
        return _case("T5-tex5x7-24x40-v2", H, W, f, views, mrm.large_triangles(5, H, W, f, *views[0], seed + 5, 0.1), seed, texture_shape=(5, 7))
    B["T5-tex5x7-24x40-v2"] = free_texture
    return B


BUILDERS = _builders()
CASES = list(BUILDERS)
_MADE = {}


def make_case(name):
    if name not in _MADE:
        _MADE[name] = BUILDERS[name](7000 + 41 * CASES.index(name))
    return _MADE[name]


_MODEL_TAPS = {}


def model_taps(name):
    """the model's own tap records of a case (every view through tests/mesh_raster_model.py), and the stack of its colours: computed
    once and shared"""
    if name not in _MODEL_TAPS:
        c = make_case(name)
        Ht, Wt = c["texture"].shape[:2]
        parts, colours = [], []
        for R, t in c["views"]:
            ref = mrm.rasterise(c["vertices"], c["faces"], c["H"], c["W"], c["focal"], R, t, near=c["near"], cull=c["cull"], white=c["background"] == 1.0,
                                uvs=c["uvs"], texture=c["texture"])
            parts.append(taps_from_barycentrics(ref["bary"], ref["face_ids"], c["uvs"], Ht, Wt))
            colours.append(ref["colour"].reshape(-1, 3))
        _MODEL_TAPS[name] = ({k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, np.concatenate(colours))
    return _MODEL_TAPS[name]


# segment lengths around the default long-segment threshold (16), around the wavefront (64) and far beyond it; 0 is an empty texel
CRAFTED_LENGTHS = (0, 1, 2, 15, 16, 17, 18, 63, 64, 65, 66, 0, 127, 128, 129, 4097, 0, 100003, 1, 16, 17, 64, 65)


def crafted_list(lengths=CRAFTED_LENGTHS, num_pixels=5000, seed=99):
    """A transposed tap list made by hand, one segment of each length in ``lengths`` (texel k has lengths[k] entries): (offsets int64
    [K + 1], pixel int32 [E], weight float32 [E], grad_colour float32 [num_pixels, 3]).  Pixels ascend within a segment (wrapping
    round), weights lie in [0, 1], gradients have both signs."""
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    E = int(offsets[-1])
    pixel = np.concatenate([(np.arange(n, dtype=np.int64) * 7 + 13 * k) % num_pixels for k, n in enumerate(lengths)]).astype(np.int32) if E else np.zeros(0, np.int32)
    weight = (hash_uniform((E,), seed) * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    grad_colour = hash_uniform((num_pixels, 3), seed + 1).astype(np.float32)
    return offsets, pixel, weight, grad_colour


def crafted_reference(offsets, pixel, weight, grad_colour):
    """float64 sums and bounds [K, 3] of a crafted list"""
    K = len(offsets) - 1
    terms = weight.astype(np.float64)[:, None] * grad_colour.astype(np.float64)[pixel]
    texel = np.repeat(np.arange(K), np.diff(offsets))
    grad, mag = np.zeros((K, 3)), np.zeros((K, 3))
    np.add.at(grad, texel, terms)
    np.add.at(mag, texel, np.abs(terms))
    return grad, segment_bound(np.diff(offsets), mag)
