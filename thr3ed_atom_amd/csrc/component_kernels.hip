// component_kernels.hip -- connected components of the occupied nodes of a field (rf_label_components of relu_field.h): what
// floater removal (thr3ed_atom_amd/components.py) is built on.  DESIGN.md section 19 has the contract, the termination and
// visibility arguments and the measurements.
//
// A node is OCCUPIED iff its own activated density post(pre(D * rho)) > threshold: the predicate of rf_node_bounds, bit for bit.
// labels[n] (plain node order) = the smallest plain index of any node of n's component, -1 for an unoccupied node; sizes[r] = the
// node count of the component labelled r, 0 elsewhere.  Union-find over the lattice in three launches on the caller's stream:
//
// 1. component_local_kernel<D>: one workgroup of 512 threads per tile of 8 x 8 x 8 nodes (z fastest, one thread per node; threads
//    past the upper faces of the grid touch no memory).  The tile's labels live in LDS (2 KB), initially the node's own tile-local
//    index or -1.  A pass = every node takes the minimum over its occupied neighbours inside the tile, then every node replaces its
//    label by the root of its chain (pointer jumping); reads and writes of LDS are separated by barriers, and passes repeat until
//    __syncthreads_or says that no label fell.  Labels only ever hold indices of the node's own component and only ever fall, so
//    the fixed point is the smallest tile-local index of the piece -- which is also its smallest PLAIN index, the tile-local
//    order being the plain order restricted to the tile.  Writes labels[n] = the plain index of that root (or -1) and sizes[n] = 0.
// 2. component_merge_kernel<D>: one thread per node.  An occupied node looks at the forward half of its neighbourhood (3 / 9 / 13
//    offsets, lexicographically positive); for an occupied neighbour in ANOTHER tile it unites the two trees: find both roots,
//    atomicMin the smaller into the larger root's word, and go on from the value the atomic returned until both sides agree.
//    (A lane whose (parent of n, parent of m) equals that of the lane before it skips the pair: the other lane unites the same trees.)
//    INVARIANT labels[x] <= x, and labels[x] is a node of x's component: every chase and every unite strictly lowers the index it
//    holds, so each loop ends after finitely many steps of its own -- no thread ever waits for another one.  Other workgroups store
//    to `labels` during this launch, so every access to it here is a relaxed agent-scope atomic (loads that bypass the L1, atomicMin
//    at the L2): no stale read can occur.  (An unoccupied node's -1 is final after launch 1 and never written again.)
// 3. component_flatten_kernel: a new launch, so the forest of launch 2 is visible.  Every occupied node follows its parents to the
//    root (the smallest index of the component: the one node of the tree that no unite could lower) and stores it.  Nodes flattened
//    by other threads meanwhile hold either their old parent or their root -- both ancestors.  Then sizes[root] += 1, aggregated:
//    a wave walks 8 runs of 64 consecutive nodes; per run the lanes that share the first pending lane's root are counted with one
//    ballot, until no lane is pending.  The wave keeps the root it has met most and that root's count in registers and sends every
//    other count out as one integer atomic; at the end the four waves of the workgroup pool what they kept through LDS.  2048 nodes
//    inside one component cost one atomic, not 2048 (atomics on one address serialise: they were the whole cost of this launch
//    before the pooling).  Integer atomics: exact, order-independent.
#include "rf_device.h"

namespace {

constexpr int kComponentTile = 8;  // tile edge of launch 1 (thr3ed_atom_amd/_lib.py COMPONENT_TILE mirrors it; the tests place nodes by it)
constexpr int kComponentTileNodes = kComponentTile * kComponentTile * kComponentTile;
constexpr int kComponentBlock = 256;  // launches 2 and 3
constexpr int kFlattenChunks = 8;     // launch 3: a wave walks this many runs of 64 consecutive nodes

// (dx, dy, dz) is a neighbour offset under the connectivity whose largest L1 norm is D (1: faces, 2: + edges, 3: + corners)
template <int D>
__device__ __forceinline__ constexpr bool component_offset(int dx, int dy, int dz) {
  const int l1 = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
  return l1 >= 1 && l1 <= D;
}

__device__ __forceinline__ int label_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree, every word read at the L2 (labels[x] <= x: the index falls until it stands)
__device__ __forceinline__ int label_root(const int* labels, int x) {
  for (;;) {
    const int p = label_load(labels + x);
    if (p == x) return x;
    x = p;
  }
}

template <int D>
__global__ __launch_bounds__(kComponentTileNodes) void component_local_kernel(GridArgs g, float threshold, int* __restrict__ labels,
                                                                              int* __restrict__ sizes, int tiles_y, int tiles_z) {
  __shared__ int s_lab[kComponentTileNodes];
  const int t = threadIdx.x;
  const int lz = t & 7, ly = (t >> 3) & 7, lx = t >> 6;
  const int tile = blockIdx.x;
  const int x0 = tile / (tiles_y * tiles_z) * kComponentTile, y0 = tile / tiles_z % tiles_y * kComponentTile, z0 = tile % tiles_z * kComponentTile;
  const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
  const bool inside = x < g.X && y < g.Y && z < g.Z;
  bool occ = false;
  if (inside) {
    float pre = g.dens[(long long)node_lin(g, x, y, z) * g.dstride] * g.rho;
    if (g.mode == RF_DENSITY_ABS) pre = fabsf(pre);
    occ = density_post(pre, g.mode) > threshold;
  }
  s_lab[t] = occ ? t : -1;
  __syncthreads();
  for (;;) {
    int m = occ ? s_lab[t] : -1;
    const int cur = m;
    if (occ) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dz = -1; dz <= 1; ++dz)
            if (component_offset<D>(dx, dy, dz)) {
              const bool in_tile = (unsigned)(lx + dx) < 8u && (unsigned)(ly + dy) < 8u && (unsigned)(lz + dz) < 8u;
              if (in_tile) {
                const int v = s_lab[t + dx * 64 + dy * 8 + dz];
                if (v >= 0) m = min(m, v);
              }
            }
    }
    const bool fell = occ && m < cur;
    if (!__syncthreads_or(fell)) break;  // (the barrier also ends the reads above)
    if (fell) s_lab[t] = m;
    __syncthreads();
    int r = m;
    if (occ)
      for (int p = s_lab[r]; p != r; p = s_lab[r]) r = p;  // (read-only phase; s_lab[r] <= r)
    __syncthreads();
    if (occ) s_lab[t] = r;
    __syncthreads();
  }
  if (inside) {
    const long long n = ((long long)x * g.Y + y) * g.Z + z;
    int out = -1;
    if (occ) {
      const int r = s_lab[t];
      out = (int)(((long long)(x0 + (r >> 6)) * g.Y + (y0 + ((r >> 3) & 7))) * g.Z + (z0 + (r & 7)));
    }
    labels[n] = out;
    if (sizes) sizes[n] = 0;
  }
}

template <int D>
__global__ __launch_bounds__(kComponentBlock) void component_merge_kernel(int X, int Y, int Z, int* labels, long long nodes) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  int x = 0, y = 0, z = 0, ln = -1;  // ln: the parent of n as launch 1 left it or lower -- an ancestor of n whenever it was read
  if (n < nodes) {
    z = (int)(n % Z), y = (int)((n / Z) % Y), x = (int)(n / ((long long)Z * Y));
    // only a node on a face of its tile has a neighbour in another one
    if ((x & 7) == 7 || ((y + 1) & 7) <= 1 || ((z + 1) & 7) <= 1) ln = label_load(labels + n);
  }
  if (__ballot(ln >= 0) == 0ull) return;  // (wave-uniform: the shuffles below need the whole wave)
  int mine = -1;  // an ancestor of n, found once and lowered by every unite (a unite may start from any node of a tree)
#pragma unroll
  for (int dx = 0; dx <= 1; ++dx)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        const bool forward = dx == 1 || (dy == 1 || (dy == 0 && dz == 1));
        if (!forward || !component_offset<D>(dx, dy, dz)) continue;  // (compile time)
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        int lm = -1;  // the parent of the neighbour m, when m exists, lies in another tile (launch 1 united the tile) and is occupied
        if (ln >= 0 && nx < X && ny >= 0 && ny < Y && nz >= 0 && nz < Z && ((nx >> 3) != (x >> 3) || (ny >> 3) != (y >> 3) || (nz >> 3) != (z >> 3)))
          lm = label_load(labels + (((long long)nx * Y + ny) * Z + nz));
        // Uniting n with m is uniting any ancestor of n with any ancestor of m.  Along a tile face whole runs of lanes hold the same
        // pair of parents: a lane whose pair is that of the lane before it leaves the work to that lane (and so on down the run).
        const int before_ln = __shfl_up(ln, 1, kWave), before_lm = __shfl_up(lm, 1, kWave);
        if (lm < 0 || (lane > 0 && before_ln == ln && before_lm == lm)) continue;
        if (mine < 0) mine = label_root(labels, ln);
        int a = mine, b = label_root(labels, lm);
        while (a != b) {  // max(a, b) falls with every turn
          if (a < b) {
            const int s = a;
            a = b;
            b = s;
          }
          const int old = atomicMin(labels + a, b);  // the larger root under the smaller
          if (old == a) break;                       // a was a root: linked
          a = old;                                   // a had a parent already: unite that one with b
        }
        mine = min(a, b);
      }
}

__global__ __launch_bounds__(kComponentBlock) void component_flatten_kernel(int* labels, int* __restrict__ sizes, long long nodes) {
  __shared__ int s_root[kComponentBlock / kWave], s_count[kComponentBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long base = ((long long)blockIdx.x * (kComponentBlock / kWave) + wave) * (kWave * kFlattenChunks);
  int held_root = -1, held_count = 0;  // (wave-uniform) the count this wave still owes, of the root it met most so far
  for (int i = 0; i < kFlattenChunks; ++i) {
    const long long n = base + i * kWave + lane;
    int root = -1;
    if (n < nodes) {
      const int first = labels[n];  // (only this thread writes labels[n] in this launch)
      if (first >= 0) {
        root = first == (int)n ? first : label_root(labels, first);
        if (root != first) labels[n] = root;
      }
    }
    if (!sizes) continue;
    bool pending = root >= 0;
    unsigned long long todo = __ballot(pending);
    while (todo) {  // (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int lead_root = __shfl(root, leader, kWave);
      const bool same = pending && root == lead_root;
      const unsigned long long group = __ballot(same);
      const int count = (int)__popcll(group);
      if (lead_root == held_root) {
        held_count += count;
      } else if (count > held_count) {  // the larger count stays with the wave, the smaller one goes out
        if (held_count > 0 && lane == 0) atomicAdd(sizes + held_root, held_count);
        held_root = lead_root;
        held_count = count;
      } else if (lane == 0) {
        atomicAdd(sizes + lead_root, count);
      }
      pending = pending && !same;
      todo &= ~group;
    }
  }
  if (!sizes) return;
  // the waves of the workgroup pool what they hold: equal roots go out as one atomic
  if (lane == 0) s_root[wave] = held_root, s_count[wave] = held_count;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kComponentBlock / kWave; ++w) {
      int count = s_count[w];
      if (count == 0) continue;
      for (int v = w + 1; v < kComponentBlock / kWave; ++v)
        if (s_root[v] == s_root[w]) count += s_count[v], s_count[v] = 0;
      atomicAdd(sizes + s_root[w], count);
    }
  }
}

}  // namespace

extern "C" {

int rf_label_components(const RFGrid* grid, float threshold, int32_t connectivity, int32_t* labels_dev, int32_t* sizes_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (!labels_dev) return RF_ERR_NULL_POINTER;
  if (!(threshold >= 0.0f)) return RF_ERR_BAD_SHAPE;  // (NaN fails the comparison too)
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return RF_ERR_BAD_SHAPE;
  const GridArgs g = to_args(grid);
  const long long nodes = (long long)g.X * g.Y * g.Z;
  if (nodes > 0x7fffffffLL) return RF_ERR_BAD_SHAPE;  // labels are int32 node indices
  if (labels_dev == sizes_dev) return RF_ERR_BAD_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_y = (g.Y + kComponentTile - 1) / kComponentTile, tiles_z = (g.Z + kComponentTile - 1) / kComponentTile;
  const dim3 tiles((unsigned)((g.X + kComponentTile - 1) / kComponentTile * tiles_y * tiles_z)), per_node((unsigned)((nodes + kComponentBlock - 1) / kComponentBlock));
  auto launch = [&](auto d) {
    constexpr int D = decltype(d)::value;
    hipLaunchKernelGGL(component_local_kernel<D>, tiles, dim3(kComponentTileNodes), 0, st, g, threshold, labels_dev, sizes_dev, tiles_y, tiles_z);
    hipLaunchKernelGGL(component_merge_kernel<D>, per_node, dim3(kComponentBlock), 0, st, g.X, g.Y, g.Z, labels_dev, nodes);
  };
  if (connectivity == 6) launch(std::integral_constant<int, 1>{});
  else if (connectivity == 18) launch(std::integral_constant<int, 2>{});
  else launch(std::integral_constant<int, 3>{});
  const long long per_block = (long long)kComponentBlock * kFlattenChunks;
  hipLaunchKernelGGL(component_flatten_kernel, dim3((unsigned)((nodes + per_block - 1) / per_block)), dim3(kComponentBlock), 0, st, labels_dev, sizes_dev, nodes);
  return launch_status();
}

}  // extern "C"
