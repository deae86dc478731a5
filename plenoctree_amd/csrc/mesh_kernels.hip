// Isosurface meshing on the device (gfx950): marching cubes on a dense float32 grid, and the sampler that puts a PlenOctree's
// sigma onto such a grid.  Entry points: pxo_mc_workspace_bytes / pxo_mc_count / pxo_mc_emit / pxo_tree_sigma_grid /
// pxo_mc_vertex_gradients / pxo_shade_points (include/plenoctree_octree.h, "isosurface meshing"); definition and output order are those of
// plenoctree_amd/nerf_sh/isosurface.py:marching_cubes, so the arrays compare with ==.
//
// Compiled with -ffp-contract=off (plenoctree_amd/build.py): a vertex is  index + (iso - v0) / (v1 - v0)  in float64, one IEEE
// rounding per operation as numpy evaluates it; a fused multiply-add anywhere in that chain would change the last bit.
//
// Passes, all deterministic (count -> exclusive scan -> emit, no atomics), one grid point per lane, z fastest:
//   classify   per point: the crossing flags of the three edges it owns (towards +x, +y, +z), the case index of the cell it is
//              the lower corner of, that cell's triangle count; per block (kMcBlock points) the four sums
//   scan       exclusive scan of the four block-sum arrays: tile sums (kMcScanTile block sums per tile), a scan of the tile
//              sums by one workgroup, then every tile scans itself in place
//   vertices   rank inside the wave from a 64-bit ballot + popcount, wave totals through LDS, block offset from the scan:
//              writes the vertex, its inside end point and its id into the dense per-axis id array
//   triangles  wave scan of the triangle counts; every triangle looks its three edges' ids up in the id arrays
//
// Per-vertex attributes, one vertex per lane (the reference's gen_mesh.py:77-82 has no colour flag, and its save_obj, :133-158,
// takes a vert_rgb that no caller passes: "# TODO: implement color"):
//   pxo_mc_vertex_gradients  the sigma gradient at every vertex (isosurface.py:vertex_gradients, float64, compares with ==)
//   pxo_shade_points         sigmoid of the SH or SG sum of a coefficient row along a direction, float32
#include "pxo_common.h"
#include "pxo_sh.h"
#include "../../include/plenoctree_octree.h"

namespace pxo {

constexpr int kMcBlock = 256;        // grid points per workgroup (4 waves, one point per lane)
constexpr int kMcWaves = kMcBlock / 64;
constexpr int kMcScanTile = 1024;    // block sums per scan tile (256 threads x 4)
constexpr int kMcTriMax = 5;         // triangles per cell: the row length of the uploaded case table
constexpr int kMcCounters = 4;       // crossing edges along x, y, z; triangles
constexpr int kSigmaGridMaxPad = 64;

// workspace carving (bytes, every section 256-byte aligned); N grid points, nb = ceil(N / kMcBlock), nt = ceil(nb / kMcScanTile)
//   ids    3 x int32 [N]     global vertex id of the edge a point owns along each axis (written where the edge crosses)
//   cases  uint8 [N]         case index of the cell whose lower corner the point is (0 where there is no such cell)
//   flags  uint8 [N]         bit a: the edge towards +axis a crosses; bit 3: the point is the lower corner of a cell;
//                            bits 4-6: that cell's triangle count (the emit passes need one byte per point to find their work)
//   bsum   uint32 [4, nb]    block sums, scanned in place to exclusive block offsets
//   tsum   int64 [4, nt]     tile sums, scanned in place to exclusive tile offsets
//   totals int64 [4]
struct McWs {
  int64_t n, nb, nt;
  int64_t id_off[3], case_off, flag_off, bsum_off, tsum_off, total_off, total;
};

static bool mc_points(int nx, int ny, int nz, int64_t* n) {
  const __int128 t = (__int128)nx * ny * nz;
  if (t >= ((__int128)1 << 31)) return false;
  *n = (int64_t)t;
  return true;
}

static McWs mc_ws(int64_t n) {
  McWs w{};
  w.n = n;
  w.nb = (n + kMcBlock - 1) / kMcBlock;
  w.nt = (w.nb + kMcScanTile - 1) / kMcScanTile;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off += (bytes + 255) & ~(int64_t)255; return o; };
  for (int a = 0; a < 3; ++a) w.id_off[a] = take(4 * n);
  w.case_off = take(n);
  w.flag_off = take(n);
  w.bsum_off = take(4 * kMcCounters * w.nb);
  w.tsum_off = take(8 * kMcCounters * w.nt);
  w.total_off = take(8 * kMcCounters);
  w.total = off;
  return w;
}

__device__ inline int mc_lane() { return threadIdx.x & 63; }
__device__ inline int mc_wave() { return threadIdx.x >> 6; }

// inclusive scan over the 64 lanes of a wave
__device__ inline uint32_t wave_incl_scan(uint32_t v) {
  const int lane = mc_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ inline int64_t wave_incl_scan64(int64_t v) {
  const int lane = mc_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

struct McGrid {
  int nx, ny, nz;
  int64_t n, sx, sy;           // points; stride of x (ny * nz) and of y (nz); z has stride 1
};

// p < n < 2^31 (mc_points): 32-bit divisions, a fraction of the instructions of 64-bit ones
__device__ inline void mc_coords(const McGrid& g, int64_t p, int& x, int& y, int& z) {
  const uint32_t q = (uint32_t)p / (uint32_t)g.nz;
  z = (int)((uint32_t)p - q * (uint32_t)g.nz);
  x = (int)(q / (uint32_t)g.ny);
  y = (int)(q - (uint32_t)x * (uint32_t)g.ny);
}

__global__ __launch_bounds__(kMcBlock) void mc_classify_kernel(const float* __restrict__ vol, McGrid g, float iso,
                                                               const uint8_t* __restrict__ tri_count,
                                                               uint8_t* __restrict__ cases, uint8_t* __restrict__ flags,
                                                               uint32_t* __restrict__ bsum, int64_t nb) {
  __shared__ uint32_t wsum[kMcWaves][kMcCounters];
  const int64_t p = blockIdx.x * (int64_t)kMcBlock + threadIdx.x;
  uint32_t ef = 0, cs = 0, ntri = 0;
  if (p < g.n) {
    int x, y, z;
    mc_coords(g, p, x, y, z);
    const bool hx = x + 1 < g.nx, hy = y + 1 < g.ny, hz = z + 1 < g.nz;
    const uint32_t i0 = vol[p] >= iso;
    const uint32_t ix = hx ? vol[p + g.sx] >= iso : i0;
    const uint32_t iy = hy ? vol[p + g.sy] >= iso : i0;
    const uint32_t iz = hz ? vol[p + 1] >= iso : i0;
    ef = (uint32_t)(ix != i0) | (uint32_t)(iy != i0) << 1 | (uint32_t)(iz != i0) << 2;
    if (hx && hy && hz) {                      // corner c = dx + 2 dy + 4 dz
      const uint32_t ixy = vol[p + g.sx + g.sy] >= iso, ixz = vol[p + g.sx + 1] >= iso;
      const uint32_t iyz = vol[p + g.sy + 1] >= iso, ixyz = vol[p + g.sx + g.sy + 1] >= iso;
      cs = i0 | ix << 1 | iy << 2 | ixy << 3 | iz << 4 | ixz << 5 | iyz << 6 | ixyz << 7;
      ntri = min((uint32_t)tri_count[cs], (uint32_t)kMcTriMax);
      ef |= 8u | ntri << 4;
    }
    cases[p] = (uint8_t)cs;
    flags[p] = (uint8_t)ef;
  }
  const int lane = mc_lane(), wave = mc_wave();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint64_t b = __ballot((ef >> a) & 1u);
    if (lane == 0) wsum[wave][a] = (uint32_t)__popcll(b);
  }
  uint32_t t = ntri;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
  if (lane == 0) wsum[wave][3] = t;
  __syncthreads();
  if (threadIdx.x < kMcCounters) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kMcWaves; ++w) s += wsum[w][threadIdx.x];
    bsum[threadIdx.x * nb + blockIdx.x] = s;
  }
}

// grid (nt, 4): tsum[c][tile] = sum of the tile's block sums
__global__ __launch_bounds__(256) void mc_tile_sum_kernel(const uint32_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ tsum,
                                                          int64_t nt) {
  __shared__ uint32_t wsum[4];
  const int c = blockIdx.y;
  const int64_t i0 = blockIdx.x * (int64_t)kMcScanTile + threadIdx.x * 4;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < nb) s += bsum[c * nb + i0 + k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (mc_lane() == 0) wsum[mc_wave()] = s;
  __syncthreads();
  if (threadIdx.x == 0) tsum[c * nt + blockIdx.x] = (int64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup of 4 waves, wave c scans counter c's tile sums in place (exclusive) and writes its total
__global__ __launch_bounds__(256) void mc_tile_scan_kernel(int64_t* __restrict__ tsum, int64_t nt, int64_t* __restrict__ totals) {
  const int c = mc_wave(), lane = mc_lane();
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < nt; i0 += 64) {
    const int64_t i = i0 + lane;
    const int64_t v = i < nt ? tsum[c * nt + i] : 0;
    const int64_t incl = wave_incl_scan64(v);
    if (i < nt) tsum[c * nt + i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) totals[c] = carry;
}

// grid (nt, 4): exclusive scan of a tile's block sums in place, offset by the tile's own exclusive offset.  Offsets are kept
// in 32 bits: they are only used when every total is below 2^31 (pxo_mc_emit refuses otherwise).
__global__ __launch_bounds__(256) void mc_block_scan_kernel(uint32_t* __restrict__ bsum, int64_t nb, const int64_t* __restrict__ tsum,
                                                            int64_t nt) {
  __shared__ uint32_t wsum[4];
  const int c = blockIdx.y;
  const int64_t i0 = blockIdx.x * (int64_t)kMcScanTile + threadIdx.x * 4;
  uint32_t v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = i0 + k < nb ? bsum[c * nb + i0 + k] : 0u;
    s += v[k];
  }
  const uint32_t incl = wave_incl_scan(s);
  if (mc_lane() == 63) wsum[mc_wave()] = incl;
  __syncthreads();
  uint32_t off = (uint32_t)tsum[c * nt + blockIdx.x] + incl - s;
  for (int w = 0; w < mc_wave(); ++w) off += wsum[w];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < nb) bsum[c * nb + i0 + k] = off;
    off += v[k];
  }
}

struct McIds {
  int32_t* a[3];
};

__global__ __launch_bounds__(kMcBlock) void mc_vertex_kernel(const float* __restrict__ vol, McGrid g, double iso, float isof,
                                                             const uint8_t* __restrict__ flags, const uint32_t* __restrict__ boff,
                                                             int64_t nb, int64_t base_y, int64_t base_z, int64_t n_vert, McIds ids,
                                                             double* __restrict__ vertices, int64_t* __restrict__ inside_idx) {
  __shared__ uint32_t wsum[3][kMcWaves];
  const int64_t p = blockIdx.x * (int64_t)kMcBlock + threadIdx.x;
  const uint32_t ef = p < g.n ? flags[p] : 0u;
  const int lane = mc_lane(), wave = mc_wave();
  uint32_t rank[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint64_t b = __ballot((ef >> a) & 1u);
    rank[a] = (uint32_t)__popcll(b & (((uint64_t)1 << lane) - 1));
    if (lane == 0) wsum[a][wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (!(ef & 7u)) return;
  int x, y, z;
  mc_coords(g, p, x, y, z);
  const float v0 = vol[p];
  const int64_t stride[3] = {g.sx, g.sy, 1};
  const int64_t base[3] = {0, base_y, base_z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((ef >> a) & 1u)) continue;
    uint32_t r = boff[a * nb + blockIdx.x] + rank[a];
    for (int w = 0; w < wave; ++w) r += wsum[a][w];
    const int64_t id = base[a] + r;
    if (id >= n_vert) continue;                // counts that do not belong to this workspace: never write past the outputs
    ids.a[a][p] = (int32_t)id;
    const float v1 = vol[p + stride[a]];
    const double t = (iso - (double)v0) / ((double)v1 - (double)v0);
    double c[3] = {(double)x, (double)y, (double)z};
    c[a] += t;
    vertices[id * 3] = c[0];
    vertices[id * 3 + 1] = c[1];
    vertices[id * 3 + 2] = c[2];
    if (inside_idx) inside_idx[id] = v0 >= isof ? p : p + stride[a];
  }
}

// tri_table: int8 [256, kMcTriMax, 3]; an entry names a cell edge as (axis << 3 | corner offset dx + 2 dy + 4 dz of its lower end)
__global__ __launch_bounds__(kMcBlock) void mc_triangle_kernel(McGrid g, const uint8_t* __restrict__ cases,
                                                               const uint8_t* __restrict__ flags, const int8_t* __restrict__ tri_table,
                                                               const uint32_t* __restrict__ boff, int64_t n_tri, McIds ids,
                                                               int64_t* __restrict__ triangles) {
  __shared__ uint32_t wsum[kMcWaves];
  const int64_t p = blockIdx.x * (int64_t)kMcBlock + threadIdx.x;
  const uint32_t ef = p < g.n ? flags[p] : 0u;
  const uint32_t ntri = (ef & 8u) ? min((ef >> 4) & 7u, (uint32_t)kMcTriMax) : 0u;   // as classify counted it
  const uint32_t incl = wave_incl_scan(ntri);
  if (mc_lane() == 63) wsum[mc_wave()] = incl;
  __syncthreads();
  if (ntri == 0) return;
  const uint32_t cs = cases[p];
  int64_t t0 = (int64_t)boff[blockIdx.x] + incl - ntri;
  for (int w = 0; w < mc_wave(); ++w) t0 += wsum[w];
  for (uint32_t t = 0; t < ntri; ++t) {
    if (t0 + t >= n_tri) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int code = tri_table[(cs * kMcTriMax + t) * 3 + k];
      const int a = min((code >> 3) & 3, 2);
      const int64_t q = p + ((code & 1) ? g.sx : 0) + ((code & 2) ? g.sy : 0) + ((code & 4) ? 1 : 0);
      triangles[(t0 + t) * 3 + k] = ids.a[a][q];
    }
  }
}

// Sigma (and the packed leaf index) of the tree at the centres of the 2^depth cells per axis, padded by `pad` layers.  The
// centre of cell i along an axis is (i + 1/2) / 2^depth: its binary digits are the `depth` bits of i, then a one, then zeros,
// so the descent picks its child from those digits and no float coordinate is formed.
__global__ __launch_bounds__(256) void tree_sigma_grid_kernel(const int32_t* __restrict__ child, const float* __restrict__ data,
                                                              int64_t n_internal, int data_dim, int depth, int pad, int side,
                                                              int64_t n, float* __restrict__ sigma, int64_t* __restrict__ packed) {
  const int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (p >= n) return;
  // q < side^2 < 2^23 always; p itself leaves 32 bits only for the grids of depth 11
  const uint32_t q = n <= 0xffffffffll ? (uint32_t)p / (uint32_t)side : (uint32_t)(p / side);
  const int k = (int)(p - (int64_t)q * side) - pad;
  const uint32_t qi = q / (uint32_t)side;
  const int i = (int)qi - pad;
  const int j = (int)(q - qi * (uint32_t)side) - pad;
  const int reso = 1 << depth;
  float s = 0.0f;
  int64_t leaf = -1;
  if (i >= 0 && j >= 0 && k >= 0 && i < reso && j < reso && k < reso) {
    int64_t node = 0;
    for (int lvl = 0; lvl <= PXO_TREE_MAX_DEPTH + 1; ++lvl) {
      const int b = depth - 1 - lvl;
      int cell;
      if (b >= 0) cell = (((i >> b) & 1) * 2 + ((j >> b) & 1)) * 2 + ((k >> b) & 1);
      else cell = b == -1 ? 7 : 0;
      const int32_t skip = child[node * 8 + cell];
      if (skip == 0) {
        leaf = node * 8 + cell;
        break;
      }
      node += skip;
      if (node < 0 || node >= n_internal) break;   // a malformed child array: report -1, read nothing out of range
    }
    if (leaf >= 0) s = data[leaf * data_dim + data_dim - 1];
  }
  sigma[p] = s;
  if (packed) packed[p] = leaf;
}

// ---- what turns the mesh into an asset: a normal and a colour per vertex (the reference's gen_mesh.py:77-82 defines no colour
// flag and its save_obj, :133-158, is never handed one: "# TODO: implement color") ------------------------------------------
constexpr int kVgBlock = 256;        // vertices per workgroup of the gradient kernel, points per workgroup of the shader

// g(p)[a] of isosurface.py:vertex_gradients: the central difference halved where both neighbours exist, the one-sided
// difference at a border.  float64 from the float32 samples, one rounding per operation.
__device__ inline double mc_point_gradient(const float* __restrict__ vol, int64_t p, int c, int extent, int64_t stride) {
  const bool lo = c > 0, hi = c + 1 < extent;
  const double d = (double)vol[hi ? p + stride : p] - (double)vol[lo ? p - stride : p];
  return lo && hi ? d * 0.5 : d;
}

// One vertex per lane.  The vertex's edge is found from what the emit pass left: inside_idx names one end point q of the edge;
// the edge is (q, q + e_a) if that edge crosses and carries this vertex's id in the id array of its axis, else (q - e_a, q).
// (An inside point between two outside ones owns a vertex on either side, so the flag alone does not decide.)  An inside_idx
// that names no such edge -- not this workspace's -- gives a zero gradient and reads nothing out of range.
__global__ __launch_bounds__(kVgBlock) void mc_vertex_gradient_kernel(const float* __restrict__ vol, McGrid g, double iso,
                                                                      const uint8_t* __restrict__ flags, McIds ids,
                                                                      const int64_t* __restrict__ inside_idx, int64_t base_y,
                                                                      int64_t base_z, int64_t n_vert,
                                                                      double* __restrict__ gradients) {
  const int64_t id = blockIdx.x * (int64_t)kVgBlock + threadIdx.x;
  if (id >= n_vert) return;
  const int a = id < base_y ? 0 : (id < base_z ? 1 : 2);
  const int64_t stride = a == 0 ? g.sx : (a == 1 ? g.sy : 1);
  const int64_t q = inside_idx[id];
  double out[3] = {0.0, 0.0, 0.0};
  if (q >= 0 && q < g.n) {
    int64_t lo = -1;
    if (((flags[q] >> a) & 1u) && ids.a[a][q] == (int32_t)id) lo = q;
    else if (q >= stride && ((flags[q - stride] >> a) & 1u) && ids.a[a][q - stride] == (int32_t)id) lo = q - stride;
    if (lo >= 0) {
      int c[3];
      mc_coords(g, lo, c[0], c[1], c[2]);
      const int ext[3] = {g.nx, g.ny, g.nz};
      if (c[a] + 1 < ext[a]) {                   // always, for an edge classify flagged; keeps hi inside the grid regardless
        const int64_t hi = lo + stride;
        const int64_t st[3] = {g.sx, g.sy, 1};
        const double v0 = (double)vol[lo], v1 = (double)vol[hi];
        const double f = (iso - v0) / (v1 - v0);
        const double f0 = 1.0 - f;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const double g0 = mc_point_gradient(vol, lo, c[b], ext[b], st[b]);
          const double g1 = mc_point_gradient(vol, hi, c[b] + (b == a ? 1 : 0), ext[b], st[b]);
          out[b] = f0 * g0 + f * g1;
        }
      }
    }
  }
  gradients[id * 3] = out[0];
  gradients[id * 3 + 1] = out[1];
  gradients[id * 3 + 2] = out[2];
}

// One point per lane: out[i, c] = sigmoid(sum_k Y_k(dirs[i]) coef[r row_stride + c K + k]), r = rows ? rows[i] : i; a negative
// row is colour 0.  Y: the leaf basis of pxo_sh.h, SH without lobes, SG with them.  float32, the sum in the order of k.
template <int K>
__global__ __launch_bounds__(kVgBlock) void shade_points_kernel(const float* __restrict__ coef, int64_t row_stride,
                                                                const int64_t* __restrict__ rows, const float* __restrict__ dirs,
                                                                int64_t n, const float* __restrict__ lobes,
                                                                float* __restrict__ out_rgb) {
  const int64_t i = blockIdx.x * (int64_t)kVgBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows ? rows[i] : i;
  float rgb[3] = {0.0f, 0.0f, 0.0f};
  if (r >= 0) {
    const float x = dirs[i * 3], y = dirs[i * 3 + 1], z = dirs[i * 3 + 2];
    float Y[K];
    if (lobes) sg_basis_dyn(K, lobes, x, y, z, Y);
    else sh_basis_dyn(K, x, y, z, Y);
    const float* row = coef + r * row_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < K; ++k) s += Y[k] * row[c * K + k];
      rgb[c] = 1.0f / (1.0f + expf(-s));
    }
  }
  out_rgb[i * 3] = rgb[0];
  out_rgb[i * 3 + 1] = rgb[1];
  out_rgb[i * 3 + 2] = rgb[2];
}

static int mc_grid(const char* who, int nx, int ny, int nz, McGrid* g) {
  PXO_REQUIRE(nx >= 0 && ny >= 0 && nz >= 0, "%s: negative grid size", who);
  int64_t n = 0;
  PXO_REQUIRE(mc_points(nx, ny, nz, &n), "%s: %d x %d x %d grid points exceed the int32 vertex-id range (2^31)", who, nx, ny, nz);
  g->nx = nx; g->ny = ny; g->nz = nz;
  g->n = n;
  g->sx = (int64_t)ny * nz;
  g->sy = nz;
  return PXO_OK;
}

static bool mc_empty(const McGrid& g) { return g.nx < 2 || g.ny < 2 || g.nz < 2; }

}  // namespace pxo

using namespace pxo;

extern "C" {

int pxo_mc_workspace_bytes(int nx, int ny, int nz, size_t* bytes) {
  PXO_REQUIRE(bytes, "pxo_mc_workspace_bytes: null pointer");
  McGrid g;
  if (int rc = mc_grid("pxo_mc_workspace_bytes", nx, ny, nz, &g)) return rc;
  *bytes = mc_empty(g) ? 0 : (size_t)mc_ws(g.n).total;
  return PXO_OK;
}

int pxo_mc_count(const float* vol, int nx, int ny, int nz, double iso, const uint8_t* tri_count, void* ws, size_t ws_bytes,
                 int64_t* counts, void* stream) {
  PXO_REQUIRE(counts, "pxo_mc_count: null pointer");
  McGrid g;
  if (int rc = mc_grid("pxo_mc_count", nx, ny, nz, &g)) return rc;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  if (mc_empty(g)) return PXO_OK;
  PXO_REQUIRE(vol && tri_count && ws, "pxo_mc_count: null pointer");
  const McWs w = mc_ws(g.n);
  if (ws_bytes < (size_t)w.total) {
    set_error("pxo_mc_count: workspace %zu < %lld", ws_bytes, (long long)w.total);
    return PXO_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  uint32_t* bsum = (uint32_t*)(base + w.bsum_off);
  int64_t* tsum = (int64_t*)(base + w.tsum_off);
  int64_t* totals = (int64_t*)(base + w.total_off);
  hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, vol, g, (float)iso, tri_count,
                     (uint8_t*)(base + w.case_off), (uint8_t*)(base + w.flag_off), bsum, w.nb);
  hipLaunchKernelGGL(mc_tile_sum_kernel, dim3((unsigned)w.nt, kMcCounters), dim3(256), 0, s, (const uint32_t*)bsum, w.nb, tsum, w.nt);
  hipLaunchKernelGGL(mc_tile_scan_kernel, dim3(1), dim3(256), 0, s, tsum, w.nt, totals);
  hipLaunchKernelGGL(mc_block_scan_kernel, dim3((unsigned)w.nt, kMcCounters), dim3(256), 0, s, bsum, w.nb, (const int64_t*)tsum,
                     w.nt);
  if (int rc = check_launch("mc_count")) return rc;
  if (hipMemcpyAsync(counts, totals, sizeof(int64_t) * kMcCounters, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("pxo_mc_count: %s", hipGetErrorString(hipGetLastError()));
    return PXO_ERR_HIP;
  }
  return PXO_OK;
}

int pxo_mc_emit(const float* vol, int nx, int ny, int nz, double iso, const int8_t* tri_table, const void* ws, size_t ws_bytes,
                const int64_t* counts, double* vertices, int64_t* triangles, int64_t* inside_idx, void* stream) {
  PXO_REQUIRE(counts, "pxo_mc_emit: null pointer");
  McGrid g;
  if (int rc = mc_grid("pxo_mc_emit", nx, ny, nz, &g)) return rc;
  PXO_REQUIRE(counts[0] >= 0 && counts[1] >= 0 && counts[2] >= 0 && counts[3] >= 0, "pxo_mc_emit: negative count");
  const int64_t lim = (int64_t)1 << 31;
  PXO_REQUIRE(counts[0] < lim && counts[1] < lim && counts[2] < lim && counts[0] + counts[1] + counts[2] < lim,
              "pxo_mc_emit: %lld vertices exceed the int32 vertex-id range (2^31)",
              (long long)counts[0] + (long long)counts[1] + (long long)counts[2]);
  PXO_REQUIRE(counts[3] < lim, "pxo_mc_emit: %lld triangles exceed the int32 range (2^31)", (long long)counts[3]);
  const int64_t n_vert = counts[0] + counts[1] + counts[2], n_tri = counts[3];
  if (mc_empty(g) || (n_vert == 0 && n_tri == 0)) return PXO_OK;
  PXO_REQUIRE(vol && tri_table && ws, "pxo_mc_emit: null pointer");
  PXO_REQUIRE(n_vert == 0 || vertices, "pxo_mc_emit: null vertices");
  PXO_REQUIRE(n_tri == 0 || triangles, "pxo_mc_emit: null triangles");
  const McWs w = mc_ws(g.n);
  if (ws_bytes < (size_t)w.total) {
    set_error("pxo_mc_emit: workspace %zu < %lld", ws_bytes, (long long)w.total);
    return PXO_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  const uint32_t* boff = (const uint32_t*)(base + w.bsum_off);
  const uint8_t* flags = (const uint8_t*)(base + w.flag_off);
  McIds ids;
  for (int a = 0; a < 3; ++a) ids.a[a] = (int32_t*)(base + w.id_off[a]);
  if (n_vert > 0)
    hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, vol, g, iso, (float)iso, flags, boff, w.nb,
                       counts[0], counts[0] + counts[1], n_vert, ids, vertices, inside_idx);
  if (n_tri > 0)
    hipLaunchKernelGGL(mc_triangle_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, g, (const uint8_t*)(base + w.case_off), flags,
                       tri_table, boff + 3 * w.nb, n_tri, ids, triangles);
  return check_launch("mc_emit");
}

int pxo_mc_vertex_gradients(const float* vol, int nx, int ny, int nz, double iso, const void* ws, size_t ws_bytes,
                            const int64_t* counts, const int64_t* inside_idx, double* gradients, void* stream) {
  PXO_REQUIRE(counts, "pxo_mc_vertex_gradients: null pointer");
  McGrid g;
  if (int rc = mc_grid("pxo_mc_vertex_gradients", nx, ny, nz, &g)) return rc;
  PXO_REQUIRE(counts[0] >= 0 && counts[1] >= 0 && counts[2] >= 0 && counts[3] >= 0, "pxo_mc_vertex_gradients: negative count");
  const int64_t lim = (int64_t)1 << 31;
  PXO_REQUIRE(counts[0] < lim && counts[1] < lim && counts[2] < lim && counts[0] + counts[1] + counts[2] < lim,
              "pxo_mc_vertex_gradients: %lld vertices exceed the int32 vertex-id range (2^31)",
              (long long)counts[0] + (long long)counts[1] + (long long)counts[2]);
  PXO_REQUIRE(counts[3] < lim, "pxo_mc_vertex_gradients: %lld triangles exceed the int32 range (2^31)", (long long)counts[3]);
  const int64_t n_vert = counts[0] + counts[1] + counts[2];
  if (mc_empty(g) || n_vert == 0) return PXO_OK;
  PXO_REQUIRE(vol && ws && inside_idx && gradients, "pxo_mc_vertex_gradients: null pointer");
  const McWs w = mc_ws(g.n);
  if (ws_bytes < (size_t)w.total) {
    set_error("pxo_mc_vertex_gradients: workspace %zu < %lld", ws_bytes, (long long)w.total);
    return PXO_ERR_WORKSPACE;
  }
  char* base = (char*)ws;
  McIds ids;
  for (int a = 0; a < 3; ++a) ids.a[a] = (int32_t*)(base + w.id_off[a]);
  hipLaunchKernelGGL(mc_vertex_gradient_kernel, dim3((unsigned)((n_vert + kVgBlock - 1) / kVgBlock)), dim3(kVgBlock), 0,
                     (hipStream_t)stream, vol, g, iso, (const uint8_t*)(base + w.flag_off), ids, inside_idx, counts[0],
                     counts[0] + counts[1], n_vert, gradients);
  return check_launch("mc_vertex_gradients");
}

int pxo_shade_points(const float* coef, int64_t row_stride, const int64_t* rows, const float* dirs, int64_t n, int basis_dim,
                     const float* lobes, float* out_rgb, void* stream) {
  PXO_REQUIRE(basis_dim == 1 || basis_dim == 4 || basis_dim == 9 || basis_dim == 16 || basis_dim == 25,
              "pxo_shade_points: basis_dim %d not in {1, 4, 9, 16, 25}", basis_dim);
  PXO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "pxo_shade_points: %lld points outside [0, 2^31)", (long long)n);
  PXO_REQUIRE(row_stride >= 3 * (int64_t)basis_dim, "pxo_shade_points: row_stride %lld < 3 * basis_dim = %d",
              (long long)row_stride, 3 * basis_dim);
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(coef && dirs && out_rgb, "pxo_shade_points: null pointer");
  const dim3 grid((unsigned)((n + kVgBlock - 1) / kVgBlock)), block(kVgBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (basis_dim) {
#define PXO_SHADE_CASE(K)                                                                                                   \
    case K: hipLaunchKernelGGL(shade_points_kernel<K>, grid, block, 0, s, coef, row_stride, rows, dirs, n, lobes, out_rgb); \
      break;
    PXO_SHADE_CASE(1) PXO_SHADE_CASE(4) PXO_SHADE_CASE(9) PXO_SHADE_CASE(16) PXO_SHADE_CASE(25)
#undef PXO_SHADE_CASE
  }
  return check_launch("shade_points");
}

int pxo_tree_sigma_grid(const PxoTree* tree, int depth, int pad, float* sigma, int64_t* packed, void* stream) {
  PXO_REQUIRE(tree && sigma, "pxo_tree_sigma_grid: null pointer");
  PXO_REQUIRE(tree->child && tree->data && tree->n_internal >= 1 && tree->data_dim >= 1, "pxo_tree_sigma_grid: empty tree");
  PXO_REQUIRE(depth >= 1 && depth <= PXO_TREE_MAX_DEPTH + 1, "pxo_tree_sigma_grid: depth %d outside [1,%d]", depth,
              PXO_TREE_MAX_DEPTH + 1);
  PXO_REQUIRE(pad >= 0 && pad <= kSigmaGridMaxPad, "pxo_tree_sigma_grid: pad %d outside [0,%d]", pad, kSigmaGridMaxPad);
  const int side = (1 << depth) + 2 * pad;
  const int64_t n = (int64_t)side * side * side;
  hipLaunchKernelGGL(tree_sigma_grid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tree->child,
                     tree->data, tree->n_internal, tree->data_dim, depth, pad, side, n, sigma, packed);
  return check_launch("tree_sigma_grid");
}

}  // extern "C"
