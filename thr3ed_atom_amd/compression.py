"""Vector-quantised compression of a trained field and the compact checkpoint it goes into (VQRF, Li et al., CVPR 2023, without its
fine-tuning step): rank the nodes by an importance score (``node_max_weights``), drop the unimportant tail, keep the important head
verbatim and quantise the feature vectors of the middle against a small codebook learnt by importance-weighted k-means.  The
k-means is the hot path -- rf_vq_assign (fused distance + argmin on the exact-f32 MFMA, the distance matrix is never in memory) and
rf_vq_centroids (csrc/vq_kernels.hip); the partition, the bit packing and ``decompress`` are ordinary numpy / torch code that runs
without a GPU, because checkpoints are loaded with ``map_location="cpu"``.  DESIGN.md section 18 has the contract, the kernels, the
error bounds and the measurements."""
import io
import json
import math
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal
from .voxels import VoxelGrid, as_kernel_grid, unpack_storage

FORMAT_VERSION = 1  # of the payload of CompressedField.to_bytes(): the "version" field of its header
VALUE_DTYPES = {"float16": np.float16, "float32": np.float32}
PRUNED, KEPT, QUANTISED = 0, 1, 2  # node classes of partition_by_shares


def _check_hip_matrix(t: Tensor, name: str) -> None:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on a HIP device: the quantiser runs on the GPU only (there is no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{name} must be a float32 matrix, got {t.dtype} {tuple(t.shape)}")


def _rows(vectors: Tensor) -> Tensor:
    """a matrix whose rows the kernels can address: unit stride inside a row, rows at least D apart (a column slice goes in as it is)"""
    M, D = vectors.shape
    if (D == 1 or vectors.stride(1) == 1) and (M <= 1 or vectors.stride(0) >= D):
        return vectors
    return vectors.contiguous()


def _check_sizes(dim: int, codes: int) -> None:
    if not 1 <= dim <= _lib.VQ_MAX_DIM:
        raise ValueError(f"vectors of 1 to {_lib.VQ_MAX_DIM} floats are supported, got {dim}")
    if not 1 <= codes <= _lib.VQ_MAX_CODES:
        raise ValueError(f"codebooks of 1 to {_lib.VQ_MAX_CODES} codes are supported, got {codes}")


def vq_assign(vectors: Tensor, codebook: Tensor) -> Tuple[Tensor, Tensor]:
    """(index int32 [M], dist float32 [M]): per row of ``vectors`` [M, D] the nearest row of ``codebook`` [C, D] by squared Euclidean
    distance (the lowest index among computed-equal ones) and that distance, recomputed for the winner as sum_k (x_k - c_k)^2 in
    ascending k.  One rf_vq_assign launch; HIP tensors only."""
    _check_hip_matrix(vectors, "vectors")
    _check_hip_matrix(codebook, "codebook")
    M, D = vectors.shape
    if codebook.shape[1] != D or codebook.device != vectors.device:
        raise ValueError(f"codebook {tuple(codebook.shape)} on {codebook.device} does not match vectors {tuple(vectors.shape)} on {vectors.device}")
    _check_sizes(D, codebook.shape[0])
    vectors, codebook = _rows(vectors.detach()), codebook.detach().contiguous()
    index = torch.empty(M, dtype=torch.int32, device=vectors.device)
    dist = torch.empty(M, dtype=torch.float32, device=vectors.device)
    stride = vectors.stride(0) if M > 1 else D
    stream = _marshal.stream(vectors.device)
    with torch.cuda.device(vectors.device):
        rc = _lib.load().rf_vq_assign(vectors.data_ptr() if M else None, M, D, stride, codebook.data_ptr(), codebook.shape[0],
                                      index.data_ptr() if M else None, dist.data_ptr() if M else None, stream)
    _lib.check(rc, "rf_vq_assign")
    return index, dist


def vq_update_centroids(vectors: Tensor, weights: Tensor, index: Tensor, codebook: Tensor) -> Tensor:
    """The weighted Lloyd update, IN PLACE on ``codebook`` [C, D]: every code that ``index`` [M] assigns vectors of positive total
    weight to becomes their weighted mean; the others keep their bits.  Returns the weight sum per code [C].  The segments come from
    a stable sort of ``index``; one rf_vq_centroids launch."""
    _check_hip_matrix(vectors, "vectors")
    _check_hip_matrix(codebook, "codebook")
    M, D = vectors.shape
    num_codes = codebook.shape[0]
    _check_sizes(D, num_codes)
    if not codebook.is_contiguous() or codebook.shape[1] != D:
        raise ValueError("codebook must be a contiguous [C, D] tensor")
    if tuple(weights.shape) != (M,) or weights.dtype != torch.float32 or tuple(index.shape) != (M,) or M >= 2**31:
        raise ValueError("weights must be float32 [M] and index an integer [M] tensor, M < 2^31")
    if M and (int(index.min()) < 0 or int(index.max()) >= num_codes):
        raise ValueError("index holds a code outside the codebook")
    vectors = _rows(vectors.detach())
    weights = weights.detach().to(vectors.device).contiguous()
    order = torch.sort(index.to(vectors.device), stable=True).indices.to(torch.int32)
    offsets = torch.zeros(num_codes + 1, dtype=torch.int64, device=vectors.device)
    offsets[1:] = torch.cumsum(torch.bincount(index.to(vectors.device, torch.int64), minlength=num_codes), 0)
    sums = torch.empty(num_codes, dtype=torch.float32, device=vectors.device)
    if M == 0:
        return sums.zero_()
    stride = vectors.stride(0) if M > 1 else D
    stream = _marshal.stream(vectors.device)
    with torch.cuda.device(vectors.device):
        rc = _lib.load().rf_vq_centroids(vectors.data_ptr(), stride, D, weights.data_ptr(), order.data_ptr(), offsets.data_ptr(), num_codes,
                                         codebook.data_ptr(), sums.data_ptr(), stream)
    _lib.check(rc, "rf_vq_centroids")
    return sums


def vq_kmeans(vectors: Tensor, weights: Tensor, num_codes: int, iterations: int = 10, seed: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """Importance-weighted k-means of ``vectors`` [M, D] -> (codebook [C, D], index int32 [M], distortions float64 [iterations + 1]).
    ``num_codes`` is capped at M.  The initial codebook is the vectors at the first C entries of ``torch.randperm(M)`` drawn from a
    CPU generator seeded with ``seed``; every iteration is an assignment followed by a centroid update, and a final assignment makes
    ``index`` belong to the returned codebook.  ``distortions[i]`` = sum w dist / sum w of assignment i, summed in float64 on the
    device.  Nothing in it is atomic or unordered: the same inputs and seed give a bit-identical codebook and index."""
    _check_hip_matrix(vectors, "vectors")
    M, D = vectors.shape
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must not be negative")
    if tuple(weights.shape) != (M,) or weights.dtype != torch.float32:
        raise ValueError(f"weights must be a float32 [M] tensor, got {weights.dtype} {tuple(weights.shape)}")
    num_codes = min(int(num_codes), M)
    if M == 0:
        return vectors.new_zeros((0, D)), torch.zeros(0, dtype=torch.int32, device=vectors.device), torch.zeros(iterations + 1, dtype=torch.float64, device=vectors.device)
    _check_sizes(D, num_codes)
    with torch.no_grad():
        vectors = _rows(vectors.detach())
        weights = weights.detach().to(vectors.device).contiguous()
        generator = torch.Generator(device="cpu")
        generator.manual_seed(int(seed))
        first = torch.randperm(M, generator=generator)[:num_codes].to(vectors.device)
        codebook = vectors[first].contiguous()
        w64 = weights.double()
        total = w64.sum()
        distortions = []
        for _ in range(iterations):
            index, dist = vq_assign(vectors, codebook)
            distortions.append((w64 * dist.double()).sum() / total)
            vq_update_centroids(vectors, weights, index, codebook)
        index, dist = vq_assign(vectors, codebook)
        distortions.append((w64 * dist.double()).sum() / total)
    return codebook, index, torch.stack(distortions)


def partition_by_shares(importance, prune_share: float, keep_share: float) -> np.ndarray:
    """The class (PRUNED, KEPT or QUANTISED) of every node, uint8 in node order.  The nodes are ranked by importance, the more
    important first and the lower node index first among equals, and the importances are accumulated along that ranking in float64,
    one after the other.  PRUNED: the inclusive sum from the least important node up to and including the node is at most
    ``prune_share`` x total (a node of importance 0 is always pruned).  KEPT: not pruned, and the sum over the nodes ranked before it
    is below ``keep_share`` x total.  QUANTISED: the rest."""
    imp = np.asarray(importance.detach().cpu().numpy() if isinstance(importance, Tensor) else importance, dtype=np.float64).reshape(-1)
    if not (0.0 <= float(prune_share) <= 1.0 and 0.0 <= float(keep_share) <= 1.0):
        raise ValueError("prune_share and keep_share must lie in [0, 1]")
    if imp.size and not (np.isfinite(imp).all() and imp.min() >= 0.0):
        raise ValueError("importance must be finite and non-negative")
    rank = np.argsort(-imp, kind="stable")
    ranked = imp[rank]
    from_below = np.cumsum(ranked[::-1])[::-1]          # inclusive, from the least important node up
    total = float(from_below[0]) if imp.size else 0.0
    before = np.concatenate([[0.0], np.cumsum(ranked)[:-1]])  # exclusive, from the most important node down
    pruned = from_below <= float(prune_share) * total
    kept = ~pruned & (before < float(keep_share) * total)
    classes = np.empty(imp.size, dtype=np.uint8)
    classes[rank] = np.where(pruned, PRUNED, np.where(kept, KEPT, QUANTISED)).astype(np.uint8)
    return classes


def _pack_bits(mask: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(mask, dtype=bool).reshape(-1), bitorder="little")


def _unpack_bits(bits: np.ndarray, count: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), count=count, bitorder="little").astype(bool)


class CompressedField:
    """A field in compact form.  Holds the grid's configuration (``config``: the dictionary ``VoxelGrid.get_save_config_dict()``
    returns -- it travels beside the payload in a checkpoint), ``dims`` and ``num_features``, a bit-packed mask of the non-pruned
    nodes in plain node order (bit i of the stream = node i, least significant bit first), a bit-packed mask over the NON-PRUNED
    nodes that says which of them are quantised, the densities of the non-pruned nodes, the feature vectors of the kept nodes, the
    codebook and the uint16 code of every quantised node -- each list in node order.  Values are float16 or float32."""

    def __init__(self, dims, num_features: int, node_mask, vq_mask, densities, kept_features, codebook, indices, fill_density: float = 0.0,
                 config: Optional[Dict[str, Any]] = None, distortions=()):
        self.dims = tuple(int(v) for v in dims)
        self.num_features = int(num_features)
        nodes = self.dims[0] * self.dims[1] * self.dims[2]
        node_mask = np.asarray(node_mask, dtype=bool).reshape(-1)
        vq_mask = np.asarray(vq_mask, dtype=bool).reshape(-1)
        self.densities = np.ascontiguousarray(densities).reshape(-1)
        self.kept_features = np.ascontiguousarray(kept_features).reshape(-1, self.num_features)
        self.codebook = np.ascontiguousarray(codebook).reshape(-1, self.num_features)
        self.indices = np.ascontiguousarray(indices, dtype=np.uint16).reshape(-1)
        alive, quantised = int(node_mask.sum()), int(vq_mask.sum())
        if len(self.dims) != 3 or node_mask.size != nodes or vq_mask.size != alive or self.densities.size != alive:
            raise ValueError("the masks and the densities do not match the grid's dimensions")
        if self.kept_features.shape[0] != alive - quantised or self.indices.size != quantised:
            raise ValueError("the kept features and the codes do not match the quantisation mask")
        if quantised and (self.codebook.shape[0] == 0 or int(self.indices.max()) >= self.codebook.shape[0]):
            raise ValueError("a code lies outside the codebook")
        dtypes = {a.dtype for a in (self.densities, self.kept_features, self.codebook)}
        if len(dtypes) != 1 or dtypes.pop() not in (np.dtype(np.float16), np.dtype(np.float32)):
            raise ValueError("densities, kept features and codebook must share one of the dtypes float16, float32")
        self.node_bits, self.vq_bits = _pack_bits(node_mask), _pack_bits(vq_mask)
        self.counts = {"pruned": nodes - alive, "kept": alive - quantised, "quantised": quantised}
        self.fill_density = float(fill_density)
        self.config = config
        self.distortions = [float(v) for v in distortions]
        self._payload_bytes: Optional[int] = None

    @property
    def value_dtype(self) -> str:
        return str(self.densities.dtype)

    @property
    def stats(self) -> Dict[str, Any]:
        """node counts per class, codebook size, the bytes of ``to_bytes()`` and the weighted distortion of the final assignment"""
        if self._payload_bytes is None:
            self._payload_bytes = len(self.to_bytes())
        return dict(self.counts, num_codes=int(self.codebook.shape[0]), value_dtype=self.value_dtype, payload_bytes=self._payload_bytes,
                    distortion=self.distortions[-1] if self.distortions else 0.0, distortions=list(self.distortions))

    def to_bytes(self) -> bytes:
        """The arrays as ONE numpy.savez_compressed stream (deflate); the format is versioned by the "version" field of the JSON
        header inside it.  The configuration is not part of it."""
        header = {"version": FORMAT_VERSION, "dims": list(self.dims), "num_features": self.num_features, "fill_density": self.fill_density,
                  "counts": self.counts, "distortions": self.distortions}
        buffer = io.BytesIO()
        np.savez_compressed(buffer, header=np.frombuffer(json.dumps(header).encode(), dtype=np.uint8), node_bits=self.node_bits, vq_bits=self.vq_bits,
                            densities=self.densities, kept_features=self.kept_features, codebook=self.codebook, indices=self.indices)
        return buffer.getvalue()

    @classmethod
    def from_bytes(cls, data: bytes, config: Optional[Dict[str, Any]] = None) -> "CompressedField":
        with np.load(io.BytesIO(data), allow_pickle=False) as z:
            header = json.loads(bytes(z["header"]).decode())
            if header.get("version") != FORMAT_VERSION:
                raise ValueError(f"compressed field of format version {header.get('version')}; this build reads version {FORMAT_VERSION}")
            dims = header["dims"]
            node_mask = _unpack_bits(z["node_bits"], dims[0] * dims[1] * dims[2])
            vq_mask = _unpack_bits(z["vq_bits"], int(node_mask.sum()))
            field = cls(dims, header["num_features"], node_mask, vq_mask, z["densities"], z["kept_features"], z["codebook"], z["indices"],
                        header["fill_density"], config, header.get("distortions", ()))
        field._payload_bytes = len(data)
        return field

    def node_classes(self) -> np.ndarray:
        """uint8 [X * Y * Z] in node order: PRUNED, KEPT or QUANTISED"""
        nodes = self.dims[0] * self.dims[1] * self.dims[2]
        classes = np.full(nodes, PRUNED, dtype=np.uint8)
        alive = np.flatnonzero(_unpack_bits(self.node_bits, nodes))
        classes[alive] = np.where(_unpack_bits(self.vq_bits, alive.size), QUANTISED, KEPT)
        return classes

    def reference_tensors(self) -> Tuple[Tensor, Tensor]:
        """(densities [X, Y, Z, 1], features [X, Y, Z, F]), float32 on the CPU: a pruned node is the plain ``fill_density`` and zero
        features, a kept node its stored values, a quantised node ``codebook[index]``"""
        X, Y, Z = self.dims
        classes = torch.from_numpy(self.node_classes())
        densities = torch.full((X * Y * Z,), self.fill_density, dtype=torch.float32)
        features = torch.zeros((X * Y * Z, self.num_features), dtype=torch.float32)
        densities[classes != PRUNED] = torch.from_numpy(self.densities).to(torch.float32)
        features[classes == KEPT] = torch.from_numpy(self.kept_features).to(torch.float32)
        if self.indices.size:
            features[classes == QUANTISED] = torch.from_numpy(self.codebook).to(torch.float32)[torch.from_numpy(self.indices.astype(np.int64))]
        return densities.reshape(X, Y, Z, 1), features.reshape(X, Y, Z, self.num_features)

    def decompress(self, device=None, storage: str = "reference") -> VoxelGrid:
        if self.config is None:
            raise ValueError("this CompressedField carries no grid configuration: pass config= to from_bytes (a checkpoint keeps it beside the payload)")
        densities, features = self.reference_tensors()
        if device is not None:
            densities, features = densities.to(device), features.to(device)
        return VoxelGrid(densities, features, **self.config, storage=storage)


def _fill_density(mode: Optional[str], fill_density: Optional[float]) -> float:
    """the rules of prune_voxel_grid: default 0, softplus has to name one, |.| admits only 0"""
    if fill_density is None:
        if mode == "softplus":
            raise ValueError("a softplus grid has no raw density with sigma = 0: pass fill_density (e.g. -10.0)")
        fill_density = 0.0
    fill_density = float(fill_density)
    if math.isnan(fill_density):
        raise ValueError("fill_density must not be NaN")
    if mode == "abs" and fill_density != 0.0:
        raise ValueError("under the |.| density activation the only fill is 0")
    return fill_density


def compress_voxel_grid(grid_or_model, importance: Tensor, *, prune_share: float = 0.001, keep_share: float = 0.6, num_codes: int = 4096, iterations: int = 10,
                        value_dtype: str = "float16", fill_density: Optional[float] = None, seed: int = 0) -> CompressedField:
    """Compress a field by importance (``node_max_weights``; any non-negative float32 [X, Y, Z] tensor in plain node order):
    ``partition_by_shares`` sorts the nodes into pruned / kept / quantised, the F feature channels of the quantised nodes are
    gathered into one [M, F] tensor from whatever storage the grid has and quantised by ``vq_kmeans`` with the importances as weights
    against ``num_codes`` (at most 65536) codes.  Densities of all non-pruned nodes, the kept nodes' features and the codebook are
    stored in ``value_dtype`` ("float16" or "float32").  The grid is not changed.  Works on every storage and on any VoxelGrid-like
    module; the quantiser needs the grid on a HIP device (a partition without quantised nodes does not)."""
    module = getattr(grid_or_model, "thre3d_repr", grid_or_model)
    grid = as_kernel_grid(module)
    if value_dtype not in VALUE_DTYPES:
        raise ValueError(f"value_dtype must be one of {sorted(VALUE_DTYPES)}")
    if not 1 <= int(num_codes) <= _lib.VQ_MAX_CODES:
        raise ValueError(f"num_codes must lie in [1, {_lib.VQ_MAX_CODES}] (the codes are stored as uint16)")
    try:
        mode = grid.density_mode
    except ValueError:
        mode = None
    fill = _fill_density(mode, fill_density)
    dims = tuple(int(v) for v in grid.grid_dims)
    if tuple(importance.shape) != dims:
        raise ValueError(f"importance must have the grid's dimensions {dims}, got {tuple(importance.shape)}")
    with torch.no_grad():
        first, second = grid.kernel_tensors()
        densities, features = unpack_storage(first.detach(), None if second is None else second.detach(), grid.storage, dims)
        F = int(features.shape[-1])
        densities, features = densities.reshape(-1), features.reshape(-1, F)
        classes = torch.from_numpy(partition_by_shares(importance, prune_share, keep_share)).to(densities.device)
        alive, kept, quantised = classes != PRUNED, classes == KEPT, classes == QUANTISED
        codebook, index, distortions = features.new_zeros((0, F)), torch.zeros(0, dtype=torch.int32), []
        if bool(quantised.any()):
            weights = importance.detach().to(densities.device, torch.float32).reshape(-1)[quantised].contiguous()
            codebook, index, dist = vq_kmeans(features[quantised].contiguous(), weights, int(num_codes), iterations, seed)
            distortions = dist.tolist()
        dtype = VALUE_DTYPES[value_dtype]
        field = CompressedField(dims, F, alive.cpu().numpy(), quantised[alive].cpu().numpy(), densities[alive].cpu().numpy().astype(dtype),
                                features[kept].cpu().numpy().astype(dtype), codebook.cpu().numpy().astype(dtype), index.cpu().numpy().astype(np.uint16),
                                fill, module.get_save_config_dict() if hasattr(module, "get_save_config_dict") else None, distortions)
    return field
