// PlenOctree side of the path on gfx950: N3Tree build from the grid mask, leaf sampling, the
// training-view weight mask over the dense grid, the octree volume renderer (forward + gradient), and the forward
// renderer of compressed trees read through their palettes (octree_render_quant_kernel, at the end of the namespace).
// C ABI: include/plenoctree_octree.h (reference call sites cited there).
//
// This translation unit is compiled with -ffp-contract=off: the marching arithmetic (sample positions,
// cell exits, step lengths) is written one rounding per operation, so that the sequence of cells a ray
// visits does not depend on how the compiler fuses multiply-adds (oracle/octree_oracle.py takes the
// same steps in numpy float32).
//
// Tree build: with whole levels refined at a time (octree/extraction.py:341-350), svox's node order --
// breadth-first, each level sorted by packed parent cell index -- is the Morton (z-curve) order of the
// occupied cells of that level.  So the build is: occupancy pyramid stored in Morton order, one exclusive
// scan per level (rank of a cell = its node index inside the level), and the 8 children of cell m are the
// contiguous cells 8m..8m+7 of the next level.  No sort, no pointer chasing, all streams are linear.
//
// Renderer: one ray per row of ROW = 4 (the default), 8 or 16 lanes of the wave (16, 8 or 4 rays per wave64: a pixel
// patch, RowGeom).  The lanes of a row walk the tree together (uniform control flow inside a row) and share a leaf's 3*K
// coefficients: at 4 lanes per colour channel in float4 groups (KF), at 8 / 16 lanes as groups of 4 consecutive floats
// (VEC), in the 8 / 16-lane gradient kernel as single floats; the partial sums are reduced with row-local DPP shuffles.
// The node path of the previous sample is kept in LDS; the descent for the next sample resumes at the deepest node the
// two positions share instead of the root (Marcher).
// The five tree marchers (octree_render_kernel, octree_render_bwd4_kernel, octree_render_quant_kernel, octree_count_kernel,
// octree_weight_kernel) share locate_leaf (the leaf at a ray parameter and the step past it); the three renderers share
// row_ray (which ray a row of lanes takes).  The channel-aligned SH dot (octree_render_kernel, octree_render_bwd4_kernel)
// and the forward compositing (octree_render_kernel, octree_render_quant_kernel) are written out in both places: behind a
// function of any form the kernels compile to other registers and occupancies (profiles/EXPERIMENTS.md).
#include <type_traits>

#include "pxo_common.h"
#include "pxo_sh.h"
#include "../../include/plenoctree_octree.h"

namespace pxo {

constexpr int kMaxD = PXO_TREE_MAX_DEPTH;
constexpr int kBits = kMaxD + 1;             // bits per axis of the finest cell grid (2^(depth+1))

// ------------------------------------------------------------------------------------------
// Morton helpers: cell (x,y,z) of a 2^d grid <-> m, x the most significant bit of each triple
// (cell index inside a node = (i*2+j)*2+k, svox packed order).
// ------------------------------------------------------------------------------------------
__host__ __device__ inline void morton_decode(uint64_t m, int d, uint32_t& x, uint32_t& y, uint32_t& z) {
  x = y = z = 0;
  for (int b = 0; b < d; ++b) {
    const uint32_t t = (uint32_t)(m >> (3 * b)) & 7u;
    x |= ((t >> 2) & 1u) << b;
    y |= ((t >> 1) & 1u) << b;
    z |= (t & 1u) << b;
  }
}

__host__ inline int64_t pow8(int d) { return (int64_t)1 << (3 * d); }

// workspace carving (bytes): occ[1..depth], rank[1..depth], block sums, counts
struct TreeWs {
  int64_t occ_off[kMaxD + 1];
  int64_t rank_off[kMaxD + 1];
  int64_t bsum_off, count_off, total;
};
constexpr int kScanElems = 2048;             // elements per scan block (256 threads x 8 bytes)

static TreeWs tree_ws(int depth) {
  TreeWs w{};
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off += (bytes + 255) & ~(int64_t)255; return o; };
  for (int d = 1; d <= depth; ++d) w.occ_off[d] = take(pow8(d));
  for (int d = 1; d <= depth; ++d) w.rank_off[d] = take(4 * pow8(d));
  w.bsum_off = take(4 * (pow8(depth) / kScanElems + 2));
  w.count_off = take(8 * (kMaxD + 2));
  w.total = off;
  return w;
}

__global__ void threshold_mask_kernel(const float* __restrict__ v, int64_t n, float thresh, uint8_t* __restrict__ mask) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) mask[i] = v[i] >= thresh ? 1 : 0;
}

// level `depth` occupancy (Morton order) from the 2^(depth+1) mask (x slowest)
__global__ void pyramid_base_kernel(const uint8_t* __restrict__ mask, int depth, uint8_t* __restrict__ occ) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= ((int64_t)1 << (3 * depth))) return;
  uint32_t x, y, z;
  morton_decode((uint64_t)m, depth, x, y, z);
  const int64_t reso = (int64_t)2 << depth;
  uint32_t any = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t base = ((int64_t)(2 * x + (c >> 1)) * reso + (2 * y + (c & 1))) * reso + 2 * z;
    any |= *reinterpret_cast<const uint16_t*>(mask + base);   // 2z is even, reso even: 2-byte aligned
  }
  occ[m] = any ? 1 : 0;
}

__global__ void pyramid_up_kernel(const uint8_t* __restrict__ fine, int64_t n_coarse, uint8_t* __restrict__ coarse) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= n_coarse) return;
  coarse[m] = reinterpret_cast<const uint64_t*>(fine)[m] ? 1 : 0;
}

__device__ __forceinline__ uint32_t bytes_sum(uint64_t v) {       // bytes are 0/1
  return (uint32_t)__popcll(v);
}

// block-level exclusive scan of 256 per-thread counts
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave, uint32_t& block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) base += s_wave[w];
    tot += s_wave[w];
  }
  block_total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(256) void scan_blocksum_kernel(const uint8_t* __restrict__ occ, int64_t n,
                                                             uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_wave[4];
  const int64_t i8 = (blockIdx.x * (int64_t)256 + threadIdx.x) * 8;
  const uint32_t v = i8 < n ? bytes_sum(*reinterpret_cast<const uint64_t*>(occ + i8)) : 0;
  uint32_t tot;
  block_excl_scan(v, s_wave, tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// single block: in-place exclusive scan of nb block sums; total -> *count
__global__ __launch_bounds__(256) void scan_sums_kernel(uint32_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ count) {
  __shared__ uint32_t s_wave[4];
  uint32_t carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? bsum[i] : 0;
    uint32_t tot;
    const uint32_t ex = block_excl_scan(v, s_wave, tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(256) void scan_final_kernel(const uint8_t* __restrict__ occ, int64_t n,
                                                          const uint32_t* __restrict__ bsum, int32_t* __restrict__ rank) {
  __shared__ uint32_t s_wave[4];
  const int64_t i8 = (blockIdx.x * (int64_t)256 + threadIdx.x) * 8;
  const uint64_t bytes = i8 < n ? *reinterpret_cast<const uint64_t*>(occ + i8) : 0;
  uint32_t tot;
  uint32_t run = bsum[blockIdx.x] + block_excl_scan(bytes_sum(bytes), s_wave, tot);
  if (i8 >= n) return;
  int32_t r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    r[k] = (int32_t)run;
    run += (uint32_t)(bytes >> (8 * k)) & 1u;
  }
  reinterpret_cast<int4*>(rank + i8)[0] = make_int4(r[0], r[1], r[2], r[3]);
  reinterpret_cast<int4*>(rank + i8)[1] = make_int4(r[4], r[5], r[6], r[7]);
}

// nodes of depth d (cells m of level d that are occupied; d = 0: the root)
struct LevelPtrs {
  const uint8_t* occ[kMaxD + 2];
  const int32_t* rank[kMaxD + 2];
  int64_t start[kMaxD + 2];
};

__global__ void tree_emit_kernel(LevelPtrs lv, int d, int depth, int32_t* __restrict__ child,
                                 int32_t* __restrict__ parent_depth) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= ((int64_t)1 << (3 * d))) return;
  if (d > 0 && !lv.occ[d][m]) return;
  const int64_t n = d == 0 ? 0 : lv.start[d] + lv.rank[d][m];
  int32_t ch[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    ch[c] = 0;
    if (d < depth) {
      const int64_t mc = m * 8 + c;
      if (lv.occ[d + 1][mc]) ch[c] = (int32_t)(lv.start[d + 1] + lv.rank[d + 1][mc] - n);
    }
  }
  reinterpret_cast<int4*>(child + n * 8)[0] = make_int4(ch[0], ch[1], ch[2], ch[3]);
  reinterpret_cast<int4*>(child + n * 8)[1] = make_int4(ch[4], ch[5], ch[6], ch[7]);
  int64_t packed = 0;
  if (d > 0) {
    const int64_t pm = m >> 3;
    const int64_t pn = d == 1 ? 0 : lv.start[d - 1] + lv.rank[d - 1][pm];
    packed = pn * 8 + (m & 7);
  }
  parent_depth[n * 2] = (int32_t)packed;
  parent_depth[n * 2 + 1] = d;
}

// ------------------------------------------------------------------------------------------
// leaf samples
// ------------------------------------------------------------------------------------------
__global__ void tree_sample_cells_kernel(const int32_t* __restrict__ parent_depth, int64_t node0, int64_t n_nodes,
                                         int S, const float* __restrict__ u, float ox, float oy, float oz,
                                         float ix, float iy, float iz, float* __restrict__ pts) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;      // (node, cell, sample)
  if (q >= n_nodes * 8 * S) return;
  const int64_t cellq = q / S;
  int64_t node = node0 + (cellq >> 3);
  const int cell = (int)(cellq & 7);
  const int depth = parent_depth[node * 2 + 1];
  uint32_t X = (cell >> 2) & 1, Y = (cell >> 1) & 1, Z = cell & 1;
  for (int lvl = 1; lvl <= depth; ++lvl) {
    const int32_t packed = parent_depth[node * 2];
    const int c = packed & 7;
    X |= (uint32_t)((c >> 2) & 1) << lvl;
    Y |= (uint32_t)((c >> 1) & 1) << lvl;
    Z |= (uint32_t)(c & 1) << lvl;
    node = packed >> 3;
  }
  const float side = 1.0f / (float)((uint32_t)2 << depth);
  const float px = (float)X * side + u[q * 3] * side;
  const float py = (float)Y * side + u[q * 3 + 1] * side;
  const float pz = (float)Z * side + u[q * 3 + 2] * side;
  pts[q * 3] = (px - ox) / ix;
  pts[q * 3 + 1] = (py - oy) / iy;
  pts[q * 3 + 2] = (pz - oz) / iz;
}

// tree[leaf_inds].sample(S) for arbitrary leaves given by their packed cell index (node*8 + cell)
__global__ void tree_sample_leaves_kernel(const int32_t* __restrict__ parent_depth, const int64_t* __restrict__ packed,
                                          int64_t n_cells, int S, const float* __restrict__ u, float ox, float oy, float oz,
                                          float ix, float iy, float iz, float* __restrict__ pts) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;      // (cell, sample)
  if (q >= n_cells * S) return;
  const int64_t pk = packed[q / S];
  int64_t node = pk >> 3;
  const int cell = (int)(pk & 7);
  const int depth = parent_depth[node * 2 + 1];
  uint32_t X = (cell >> 2) & 1, Y = (cell >> 1) & 1, Z = cell & 1;
  for (int lvl = 1; lvl <= depth; ++lvl) {
    const int32_t up = parent_depth[node * 2];
    const int c = up & 7;
    X |= (uint32_t)((c >> 2) & 1) << lvl;
    Y |= (uint32_t)((c >> 1) & 1) << lvl;
    Z |= (uint32_t)(c & 1) << lvl;
    node = up >> 3;
  }
  const float side = 1.0f / (float)((uint32_t)2 << depth);
  const float px = (float)X * side + u[q * 3] * side;
  const float py = (float)Y * side + u[q * 3 + 1] * side;
  const float pz = (float)Z * side + u[q * 3 + 2] * side;
  pts[q * 3] = (px - ox) / ix;
  pts[q * 3 + 1] = (py - oy) / iy;
  pts[q * 3 + 2] = (pz - oz) / iz;
}

// tree[points]: packed index (node*8 + cell) of the leaf containing each world-space point.  svox's query: tree
// coordinates clamped to [0, 1 - 1e-6], then per level x *= 2, cell = floor(x), x -= cell until a leaf is reached.
__global__ void tree_query_kernel(const int32_t* __restrict__ child, const float* __restrict__ pts, int64_t n, float ox,
                                  float oy, float oz, float ix, float iy, float iz, int64_t* __restrict__ packed) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= n) return;
  float x = fminf(fmaxf(ox + ix * pts[q * 3], 0.0f), 1.0f - 1e-6f);
  float y = fminf(fmaxf(oy + iy * pts[q * 3 + 1], 0.0f), 1.0f - 1e-6f);
  float z = fminf(fmaxf(oz + iz * pts[q * 3 + 2], 0.0f), 1.0f - 1e-6f);
  int64_t node = 0;
  for (int lvl = 0; lvl <= kMaxD + 1; ++lvl) {
    x *= 2.0f; y *= 2.0f; z *= 2.0f;
    const int i = (int)floorf(x), j = (int)floorf(y), k = (int)floorf(z);
    x -= (float)i; y -= (float)j; z -= (float)k;
    const int cell = (i * 2 + j) * 2 + k;
    const int32_t skip = child[node * 8 + cell];
    if (skip == 0) {
      packed[q] = node * 8 + cell;
      return;
    }
    node += skip;
  }
  packed[q] = -1;    // deeper than any valid tree: corrupt child array
}

__global__ void tree_relu_sigma_kernel(float* __restrict__ data, int64_t n_cells, int dim) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n_cells) {
    float& s = data[i * dim + dim - 1];
    s = fmaxf(s, 0.0f);
  }
}

// ------------------------------------------------------------------------------------------
// ray set-up shared by the marchers (svox cam2world_ray / transform_coord / _get_delta_scale / _dda_unit)
// ------------------------------------------------------------------------------------------
struct TreeRay {
  float o[3], d[3], invdir[3], vdir[3];
  float delta_scale, tmin, tmax;
};

__device__ __forceinline__ void dda_unit(const float (&cen)[3], const float (&invdir)[3], float& tmin, float& tmax) {
  tmin = 0.0f;
  tmax = 1e9f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t1 = -cen[a] * invdir[a];
    const float t2 = t1 + invdir[a];
    tmin = fmaxf(tmin, fminf(t1, t2));
    tmax = fminf(tmax, fmaxf(t1, t2));
  }
}

__device__ __forceinline__ void camera_ray(const float* __restrict__ c2w, float fx, float fy, int W, int H, int px, int py,
                                           float (&origin)[3], float (&dir)[3]) {
  float x = ((float)px - 0.5f * (float)W) / fx;
  float y = -((float)py - 0.5f * (float)H) / fy;
  float z = sqrtf((x * x + y * y) + 1.0f);
  x = x / z;
  y = y / z;
  z = -1.0f / z;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dir[a] = (c2w[a * 4] * x + c2w[a * 4 + 1] * y) + c2w[a * 4 + 2] * z;
    origin[a] = c2w[a * 4 + 3];
  }
}

__device__ __forceinline__ void to_tree_ray(const float (&origin)[3], const float (&dir)[3], const float* offset,
                                            const float* invradius, TreeRay& r) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.o[a] = offset[a] + invradius[a] * origin[a];
    r.d[a] = dir[a] * invradius[a];
  }
  const float nrm = sqrtf((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
  r.delta_scale = 1.0f / nrm;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.d[a] = r.d[a] * r.delta_scale;
    r.invdir[a] = 1.0f / (r.d[a] + 1e-9f);
  }
  dda_unit(r.o, r.invdir, r.tmin, r.tmax);
}

// NDC set-up of the pxo_*_ndc entry points (plenoctree_octree.h, items 2, 3 and 5): the world-space ray (o, d) becomes the
// unit-direction ray of normalised device coordinates, in place, between camera_ray / the explicit-ray loads and to_tree_ray.
// convert_to_ndc (octree/nerf/datasets.py:37-57) in its operation order, IEEE divisions, no contraction -- the expressions of
// ndc_row in render_kernels.hip, restated here so that that file's instruction streams stay as they are.  Returns false for a
// miss (d_z >= 0, a non-finite component, or a direction that cannot be normalised): the caller then marches nothing, so no
// NaN reaches a loop condition.  n.width == 0 marks a world-space launch (every caller tests it first: kernel-uniform).
__device__ __forceinline__ bool ndc_ray(const PxoNdc& n, float (&o)[3], float (&d)[3]) {
  const float dz = d[2];
  const float t = -(n.near + o[2]) / d[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = o[a] + t * d[a];
  const float cw = (2.f * n.focal) / (float)n.width, ch = (2.f * n.focal) / (float)n.height;
  const float ox_oz = o[0] / o[2], oy_oz = o[1] / o[2];
  const float no[3] = {-cw * ox_oz, -ch * oy_oz, 1.f + 2.f * n.near / o[2]};
  const float nd[3] = {-cw * (d[0] / d[2] - ox_oz), -ch * (d[1] / d[2] - oy_oz), -2.f * n.near / o[2]};
  const float nrm = sqrtf((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]);
  bool ok = dz < 0.0f && nrm > 0.0f && nrm < INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ok = ok && fabsf(no[a]) < INFINITY && fabsf(nd[a]) < INFINITY;       // false for NaN as well
    o[a] = no[a];
    d[a] = nd[a] / nrm;
  }
  return ok;
}

__device__ __forceinline__ float clamp_coord(float x) { return fminf(fmaxf(x, 0.0f), 1.0f - 1e-6f); }

// dda_unit for a point INSIDE the unit cell (0 <= cen < 1), as every march step calls it.  The entry distance is then
// max(0, non-positive values) = 0, and per axis the exit is max(t1, t2) with t1 = -cen * invdir, t2 = t1 + invdir: t2 when
// invdir >= 0, t1 otherwise - i.e. t1 + add with the per-ray addend add = invdir >= 0 ? invdir : 0 (t1 + 0 is t1).  Same
// operations, same roundings as dda_unit (this file is compiled without contraction), 9 instructions instead of 19.
// Returns tmax (= tmax - tmin).
// init(invdir, s) with s a POWER OF TWO returns s x the exit distance instead: scaling by 2^k commutes with every rounding of
// the mul / add / min chain (no operand gets near the under- or overflow range), so `cell_exit(local) * 2^-k` of the
// power-of-two weight-mask marchers is folded into the per-ray constants -- bit for bit the same step length, one
// multiplication per sample less.
struct CellExit {
  float inv[3], add[3], cap;
  __device__ __forceinline__ void init(const float (&invdir)[3], float pow2_scale = 1.0f) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      inv[a] = invdir[a] * pow2_scale;
      add[a] = invdir[a] >= 0.0f ? invdir[a] * pow2_scale : 0.0f;
    }
    cap = 1e9f * pow2_scale;
  }
  __device__ __forceinline__ float operator()(const float (&cen)[3]) const {
    const float e0 = -cen[0] * inv[0] + add[0];
    const float e1 = -cen[1] * inv[1] + add[1];
    const float e2 = -cen[2] * inv[2] + add[2];
    return fminf(fminf(cap, e0), fminf(e1, e2));
  }
};
// 2^-(depth+1) exactly: dividing the cell-local distance by the cell count per axis (a power of two) is this multiplication
__device__ __forceinline__ float inv_cells(int depth) { return __int_as_float((126 - depth) << 23); }

// ------------------------------------------------------------------------------------------
// grid weight render: one thread per (camera, pixel)
// ------------------------------------------------------------------------------------------
struct Vec3 { float v[3]; };

// sigma and the weights are walked in 4x4x4 bricks (256 B = two cache lines per brick): a marching ray takes
// several samples per brick and the 8x8-pixel footprint of a wave spans only a few bricks, whereas in the
// x-slowest layout nearly every sample of every lane touches its own line (PMC: 72 GB fetched per two
// cameras against 4.6 GB of 4-byte samples; profiles/r01_octree_kernels.md).
__host__ __device__ inline int64_t brick_index(int x, int y, int z, int nb) {
  return ((((int64_t)(x >> 2) * nb + (y >> 2)) * nb + (z >> 2)) << 6) | ((x & 3) << 4) | ((y & 3) << 2) | (z & 3);
}

// also counts the voxels above sigma_thresh: the weight-mask launch picks its kernel by that fraction.  Grid-stride loop, one
// atomic per wave at the END (an atomic per wave and brick -- 2 M of them on one address at 512^3 -- took 25 ms)
__global__ __launch_bounds__(256) void brick_sigma_kernel(const float* __restrict__ lin, int reso, float* __restrict__ bricked,
                                                           float sigma_thresh, unsigned long long* __restrict__ occupied) {
  const int64_t n = (int64_t)reso * reso * reso;
  const int nb = reso >> 2;
  unsigned long long count = 0;                // wave-uniform
  for (int64_t i0 = blockIdx.x * (int64_t)256; i0 < n; i0 += (int64_t)gridDim.x * 256) {   // n is a multiple of 64: waves stay whole
    const int64_t i = i0 + threadIdx.x;       // bricked index
    float v = -INFINITY;
    if (i < n) {
      const int l = (int)(i & 63);
      const int64_t b = i >> 6;
      const int bz = (int)(b % nb), by = (int)((b / nb) % nb), bx = (int)(b / ((int64_t)nb * nb));
      const int x = bx * 4 + (l >> 4), y = by * 4 + ((l >> 2) & 3), z = bz * 4 + (l & 3);
      v = lin[((int64_t)x * reso + y) * reso + z];
      bricked[i] = v;
    }
    count += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v > sigma_thresh));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(occupied, count);
}

__global__ void unbrick_max_kernel(const float* __restrict__ bricked, int reso, float* __restrict__ lin) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;       // linear index
  if (i >= (int64_t)reso * reso * reso) return;
  const int z = (int)(i % reso), y = (int)((i / reso) % reso), x = (int)(i / ((int64_t)reso * reso));
  lin[i] = fmaxf(lin[i], bricked[brick_index(x, y, z, reso >> 2)]);
}

// Which of the two weight-mask marchers runs is decided ON THE DEVICE (the call stays asynchronous; one launch, one uniform
// branch at its top).  Measured per 800x800 camera at 512^3, per-sample / slab-staged: density with fuzzy tails (97 % of the
// voxels above the threshold) 1.97 / 1.29 ms; the same spheres with exact zeros outside (6 % above) 0.95 / 1.08 ms; a NeRF
// after 105 steps (18 % above) 0.89 / 0.97 ms -- the slab marcher's staging, barriers and flush are paid per brick layer
// whether or not the rays find anything in it.
// Which 16x16-pixel tile of which camera a workgroup of the weight-mask launch takes.
//   order 0  linear: workgroup b -> camera b / tiles, tile b % tiles (row-major); consecutive workgroups go round-robin over
//            the 8 XCDs, so neighbouring tiles -- which cross the same bricks -- sit behind eight different L2s (PMC: 2.2 GB
//            read per camera against a floor of 0.46 GB)
//   order 1  XCD supertiles: the tiles of a 4x4-tile square (64x64 pixels) all go to ONE XCD (workgroup ids that are equal
//            mod 8), the squares round-robin over the XCDs, so an L2 sees whole squares and every XCD still gets every
//            part of the image.  The grid is padded (8 * ceil(squares / 8) * 16 workgroups per camera); padding returns at once.
struct GwTile { int cam, tile; };
__device__ __forceinline__ GwTile gw_tile(int64_t b, int tiles_x, int tiles_y, int order) {
  if (order == 0) {
    const int64_t tiles = (int64_t)tiles_x * tiles_y;
    return GwTile{(int)(b / tiles), (int)(b % tiles)};
  }
  const int super_x = (tiles_x + 3) >> 2, super_y = (tiles_y + 3) >> 2, nsuper = super_x * super_y;
  const int64_t per_cam = (int64_t)8 * ((nsuper + 7) >> 3) * 16;
  const int cam = (int)(b / per_cam), r = (int)(b % per_cam);
  const int xcd = r & 7, idx = r >> 3, sq = xcd + 8 * (idx >> 4), within = idx & 15;
  if (sq >= nsuper) return GwTile{cam, -1};
  const int tx = (sq % super_x) * 4 + (within & 3), ty = (sq / super_x) * 4 + (within >> 2);
  if (tx >= tiles_x || ty >= tiles_y) return GwTile{cam, -1};
  return GwTile{cam, ty * tiles_x + tx};
}
__host__ inline int64_t gw_blocks_per_cam(int tiles_x, int tiles_y, int order) {
  if (order == 0) return (int64_t)tiles_x * tiles_y;
  const int nsuper = ((tiles_x + 3) >> 2) * ((tiles_y + 3) >> 2);
  return (int64_t)8 * ((nsuper + 7) >> 3) * 16;
}

struct GwSelect {
  const unsigned long long* occupied;   // voxels above sigma_thresh (brick_sigma_kernel)
  int64_t n;                            // voxels
  int force;                            // 1: slab-staged, 0: per-sample, -1: by the occupied fraction
  int order;                            // gw_tile: 0 linear, 1 XCD supertiles
  __device__ __forceinline__ bool dense() const {
    return force >= 0 ? force != 0 : 2 * (int64_t)*occupied > n;      // more than half of the grid above the threshold
  }
};

// POW2: reso is a power of two (every grid the extraction makes): the division by it is an exact multiplication and
// the brick index is assembled from bit fields in 32 bits (reso <= 1024).
constexpr int kGwLutMax = 512;        // entries per axis of the per-sample marcher's index tables (larger grids: arithmetic)
template <bool BRICK, bool POW2>
__device__ __forceinline__ void grid_weight_body(const float* __restrict__ sigma, int reso, const float* __restrict__ c2w_all,
                                                 int n_cams, float fx, float fy, int W, int H, const PxoRenderOpts& opt,
                                                 const Vec3& offset, const Vec3& invradius, int* __restrict__ weight_bits,
                                                 const PxoNdc& ndc, uint32_t* __restrict__ s_lut = nullptr, int order = 0) {
  const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
  const GwTile gt = gw_tile(blockIdx.x, tiles_x, tiles_y, order);
  if (gt.tile < 0 || gt.cam >= n_cams) return;                 // padding of the supertile order (workgroup-uniform)
  // BRICK && POW2: the bricked index of a voxel is the OR of three per-axis bit patterns; they come from three small LDS
  // tables (s_lut: 3 x kGwLutMax words of workgroup scratch) instead of 13 shift / mask / or instructions per sample.  Filled
  // by the whole workgroup before any thread leaves.
  const bool lut = BRICK && POW2 && s_lut != nullptr && reso <= kGwLutMax;       // workgroup-uniform
  if (lut) {
    const int lbq = 31 - __clz(reso >> 2), lr = lbq + 2;               // reso = 2^lr
    for (int e = threadIdx.x; e < 3 * reso; e += blockDim.x) {
      const int a = e >> lr, x = e & (reso - 1);
      s_lut[a * kGwLutMax + x] = ((uint32_t)(x >> 2) << ((2 - a) * lbq + 6)) | ((uint32_t)(x & 3) << ((2 - a) * 2));
    }
    __syncthreads();
  }
  // 8x8 pixel tiles per 64-thread wave keep the rays of a wave in neighbouring voxels
  const int cam = gt.cam, tile = gt.tile;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
  const int py = (tile / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (cam >= n_cams || px >= W || py >= H) return;
  float origin[3], dir[3];
  camera_ray(c2w_all + (int64_t)cam * 12, fx, fy, W, H, px, py, origin, dir);
  if (ndc.width > 0 && !ndc_ray(ndc, origin, dir)) return;     // an NDC miss leaves no weight
  TreeRay r;
  to_tree_ray(origin, dir, offset.v, invradius.v, r);
  if (r.tmax < 0.0f || r.tmin > r.tmax) return;
  const float cube = (float)reso;
  const float inv_cube = 1.0f / cube;            // exact when POW2
  const int lb = 31 - __clz(reso >> 2);          // POW2: log2 of bricks per axis
  CellExit cell_exit;
  cell_exit.init(r.invdir, POW2 ? inv_cube : 1.0f);
  // POW2: the grid size is a power of two, so (o + t d) * cube == o * cube + t * (d * cube) and the clamp scales with it, bit
  // for bit (scaling by 2^k commutes with the roundings of the separate mul and add this file is compiled to): the three
  // multiplications by cube leave the loop.  r05: 47 -> 35 vector instructions per sample together with the index tables below.
  const float sc = POW2 ? cube : 1.0f;
  const float so[3] = {r.o[0] * sc, r.o[1] * sc, r.o[2] * sc}, sd[3] = {r.d[0] * sc, r.d[1] * sc, r.d[2] * sc};
  const float chi = (1.0f - 1e-6f) * sc;
  // One sample: the voxel at parameter `tt` and the step to the next sample.  Neither depends on sigma, so the march is
  // SOFTWARE-PIPELINED: the next sample's voxel is located and its sigma load issued before the current sample's sigma is
  // consumed (two loads in flight per ray; the loop was one dependent L2 / HBM round trip per sample).  Same samples, same
  // arithmetic; a ray that stops on `light <= stop_thresh` has read one sigma it did not need.
  auto locate = [&](float tt, int64_t& idx, float& delta_t) {
    float local[3];
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // (v_med3_f32: what the compiler makes of clamp_coord's constant bounds; spelled out because `chi` is a register here)
      const float p = POW2 ? __builtin_amdgcn_fmed3f(so[a] + tt * sd[a], 0.0f, chi) : clamp_coord(r.o[a] + tt * r.d[a]) * cube;
      c[a] = (int)p;                             // p >= 0: truncation == floor
      local[a] = __builtin_amdgcn_fractf(p);     // p - floor(p)
    }
    const float s1 = cell_exit(local);
    delta_t = (POW2 ? s1 : s1 / cube) + opt.step_size;
    if (BRICK && POW2) {
      const uint32_t x = (uint32_t)c[0], y = (uint32_t)c[1], z = (uint32_t)c[2];
      if (lut) idx = (uint32_t)(s_lut[x] | s_lut[kGwLutMax + y] | s_lut[2 * kGwLutMax + z]);
      else idx = (uint32_t)(((x >> 2) << (2 * lb + 6)) | ((y >> 2) << (lb + 6)) | ((z >> 2) << 6) | ((x & 3) << 4) | ((y & 3) << 2) | (z & 3));
    } else {
      idx = BRICK ? brick_index(c[0], c[1], c[2], reso >> 2) : ((int64_t)c[0] * reso + c[1]) * reso + c[2];
    }
  };
  float t = r.tmin, light = 1.0f;
  if (!(t < r.tmax)) return;
  int64_t idx;
  float delta_t;
  locate(t, idx, delta_t);
  float sg = sigma[idx];
  for (;;) {
    // the sample after this one (if the march goes on): located and requested now
    const float tn = t + delta_t;
    const bool more = tn > t && tn < r.tmax;     // !(tn > t): step below the resolution of t, stop rather than spin
    // (unconditionally: the position is clamped into the grid, so the address is valid even past tmax, and a straight-line
    // body is what lets the compiler wait for the OLDER of the two loads only -- with the request inside `if (more)` it
    // waited for both at the join and nothing overlapped)
    int64_t idx_n;
    float delta_n;
    locate(tn, idx_n, delta_n);
    const float sg_n = sigma[idx_n];
    if (sg > opt.sigma_thresh) {
      const float att = expf(-(delta_t * r.delta_scale) * sg);
      const float w = light * (1.0f - att);
      light = light * att;
      const int wb = __float_as_int(w);
      if (wb > weight_bits[idx]) atomicMax(weight_bits + idx, wb);     // w >= 0: integer order == float order
      if (light <= opt.stop_thresh) return;
    }
    if (!more) return;
    t = tn; idx = idx_n; delta_t = delta_n; sg = sg_n;
  }
}

// Slab-staged form for power-of-two bricked grids.  A workgroup is a 16x16-pixel tile whose rays sweep the grid together,
// one brick layer ("slab", 4 voxels thick along the dominant axis of the tile's centre ray) at a time: the kWin x kWin bricks
// of that layer around the centre ray are copied to LDS with 16-byte coalesced loads, every ray takes its samples of the slab
// from LDS (sigma) and folds its weights into an LDS copy of the same bricks (ds_max), and the touched weights leave as whole
// bricks (one global atomicMax per voxel and tile instead of a read and possibly an atomic per sample).  Per ray the arithmetic
// and the order of its samples are those of grid_weight_kernel, and max is order-free, so the result is bit-identical.
// Samples outside the window (rare: the window is 24 voxels wide, a tile's footprint at most ~14 + the slab's drift) and rays
// that do not advance along the sweep direction take the global path of the plain kernel.
template <int kWin>
__device__ __forceinline__ void grid_weight_slab_body(const float* __restrict__ sigma, int reso, const float* __restrict__ c2w_all,
                                                      int n_cams, float fx, float fy, int W, int H, const PxoRenderOpts& opt,
                                                      const Vec3& offset, const Vec3& invradius, int* __restrict__ weight_bits,
                                                      float* __restrict__ s_sigma, int* __restrict__ s_w, int order,
                                                      const PxoNdc& ndc) {
  __shared__ int s_first;
  const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
  const GwTile gt = gw_tile(blockIdx.x, tiles_x, tiles_y, order);
  if (gt.tile < 0 || gt.cam >= n_cams) return;                 // padding of the supertile order (workgroup-uniform)
  const int cam = gt.cam, tile = gt.tile;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tx0 = (tile % tiles_x) * 16, ty0 = (tile / tiles_x) * 16;
  const int px = tx0 + (wave & 1) * 8 + (lane & 7), py = ty0 + (wave >> 1) * 8 + (lane >> 3);
  const float* c2w = c2w_all + (int64_t)cam * 12;
  const int nb = reso >> 2, lb = 31 - __clz(nb);
  const float cube = (float)reso, inv_cube = 1.0f / cube;

  // the tile's centre ray fixes the sweep: axis A, direction sgn, and where the window sits in every slab (workgroup-uniform)
  TreeRay rc;
  {
    float oc[3], dc[3];
    camera_ray(c2w, fx, fy, W, H, min(tx0 + 8, W - 1), min(ty0 + 8, H - 1), oc, dc);
    // NDC: the sweep follows the converted centre ray.  Should that ray be a miss, any finite ray will do (the window only decides
    // which samples come from LDS); every NDC ray advances along +z, so the cube's axis is taken.
    if (ndc.width > 0 && !ndc_ray(ndc, oc, dc)) {
      oc[0] = oc[1] = 0.0f; oc[2] = -1.0f;
      dc[0] = dc[1] = 0.0f; dc[2] = 1.0f;
    }
    to_tree_ray(oc, dc, offset.v, invradius.v, rc);
  }
  const float ad0 = fabsf(rc.d[0]), ad1 = fabsf(rc.d[1]), ad2 = fabsf(rc.d[2]);
  const int A = ad0 >= ad1 && ad0 >= ad2 ? 0 : (ad1 >= ad2 ? 1 : 2), B = A == 0 ? 1 : 0, C = A == 2 ? 1 : 2;
  const int sgn = rc.d[A] >= 0.0f ? 1 : -1;
  // bit position of an axis' brick coordinate / in-brick coordinate in the bricked index (brick_index: x slowest)
  const int shA = (2 - A) * lb + 6, shB = (2 - B) * lb + 6, shC = (2 - C) * lb + 6;
  const int lsA = (2 - A) * 2, lsB = (2 - B) * 2, lsC = (2 - C) * 2;

  for (int e = tid; e < kWin * kWin * 64; e += 256) s_w[e] = 0;
  if (tid == 0) s_first = 0x7fffffff;

  // this thread's ray, axes permuted to (A, B, C)
  float po[3] = {0.f, 0.f, 0.f}, pd[3] = {0.f, 0.f, 0.f}, delta_scale = 0.0f, tmax = 0.0f, t = 0.0f, light = 1.0f;
  CellExit cell_exit;
  bool alive = cam < n_cams && px < W && py < H;
  {
    float origin[3], dir[3];
    TreeRay r;
    camera_ray(c2w, fx, fy, W, H, min(px, W - 1), min(py, H - 1), origin, dir);
    if (ndc.width > 0) alive = ndc_ray(ndc, origin, dir) && alive;       // a miss is decided here, before anything marches
    to_tree_ray(origin, dir, offset.v, invradius.v, r);
    alive = alive && !(r.tmax < 0.0f || r.tmin > r.tmax) && r.tmin < r.tmax;
    const int perm[3] = {A, B, C};
    float pinv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      po[i] = perm[i] == 0 ? r.o[0] : (perm[i] == 1 ? r.o[1] : r.o[2]);
      pd[i] = perm[i] == 0 ? r.d[0] : (perm[i] == 1 ? r.d[1] : r.d[2]);
      pinv[i] = perm[i] == 0 ? r.invdir[0] : (perm[i] == 1 ? r.invdir[1] : r.invdir[2]);
    }
    cell_exit.init(pinv, inv_cube);           // the exit distance already divided by the grid size (exact: a power of two)
    delta_scale = r.delta_scale;
    tmax = r.tmax;
    t = r.tmin;
  }
  // the ray in grid units: (o + t d) * cube == o cube + t (d cube), bit for bit, for a power-of-two cube (see grid_weight_body)
  const float so0 = po[0] * cube, so1 = po[1] * cube, so2 = po[2] * cube, sd0 = pd[0] * cube, sd1 = pd[1] * cube, sd2 = pd[2] * cube;
  const float chi = (1.0f - 1e-6f) * cube;
  // the pending sample: cell (permuted axes) and step length at the current t
  int c0 = 0, c1 = 0, c2 = 0;
  float delta_t = 0.0f;
  auto next_sample = [&]() {
    float local[3];
    const float p0 = __builtin_amdgcn_fmed3f(so0 + t * sd0, 0.0f, chi), p1 = __builtin_amdgcn_fmed3f(so1 + t * sd1, 0.0f, chi),
                p2 = __builtin_amdgcn_fmed3f(so2 + t * sd2, 0.0f, chi);
    c0 = (int)p0; c1 = (int)p1; c2 = (int)p2;
    local[0] = __builtin_amdgcn_fractf(p0); local[1] = __builtin_amdgcn_fractf(p1); local[2] = __builtin_amdgcn_fractf(p2);
    delta_t = cell_exit(local) + opt.step_size;
  };
  if (alive) next_sample();
  __syncthreads();
  if (alive) atomicMin(&s_first, (c0 >> 2) * sgn);
  __syncthreads();
  const int first = s_first;
  if (first == 0x7fffffff) return;               // no ray of the tile meets the grid (workgroup-uniform)

  const float cinvA = rc.invdir[A], coA = rc.o[A];
  const float coB = rc.o[B], cdB = rc.d[B], coC = rc.o[C], cdC = rc.d[C];
  for (int key = first;; ++key) {
    const int k = key * sgn;
    if (k < 0 || k >= nb) break;
    // window: kWin x kWin bricks of layer k around the centre ray at the layer's mid-plane
    const float tc = ((float)(4 * k + 2) * inv_cube - coA) * cinvA;
    const int wb0 = (int)floorf((coB + tc * cdB) * cube * 0.25f - 0.5f * (kWin - 1));
    const int wc0 = (int)floorf((coC + tc * cdC) * cube * 0.25f - 0.5f * (kWin - 1));
    for (int e = tid; e < kWin * kWin * 16; e += 256) {
      const int br = e >> 4, q = e & 15;
      const int bi = wb0 + br / kWin, bj = wc0 + br % kWin;
      if ((unsigned)bi < (unsigned)nb && (unsigned)bj < (unsigned)nb) {
        const uint32_t base = ((uint32_t)k << shA) | ((uint32_t)bi << shB) | ((uint32_t)bj << shC);
        *reinterpret_cast<float4*>(s_sigma + br * 64 + q * 4) = *reinterpret_cast<const float4*>(sigma + base + q * 4);
      }
    }
    __syncthreads();
    while (alive && ((c0 >> 2) - k) * sgn <= 0) {
      const int i = (c1 >> 2) - wb0, j = (c2 >> 2) - wc0;
      const bool inwin = (c0 >> 2) == k && (unsigned)i < (unsigned)kWin && (unsigned)j < (unsigned)kWin;
      const uint32_t low = ((uint32_t)(c0 & 3) << lsA) | ((uint32_t)(c1 & 3) << lsB) | ((uint32_t)(c2 & 3) << lsC);
      const int lidx = (i * kWin + j) * 64 + (int)low;
      const uint32_t gidx = ((uint32_t)(c0 >> 2) << shA) | ((uint32_t)(c1 >> 2) << shB) | ((uint32_t)(c2 >> 2) << shC) | low;
      const float sg = inwin ? s_sigma[lidx] : sigma[gidx];
      if (sg > opt.sigma_thresh) {
        const float att = expf(-(delta_t * delta_scale) * sg);
        const float w = light * (1.0f - att);
        light = light * att;
        const int wb = __float_as_int(w);                                  // w >= 0: integer order == float order
        if (inwin) atomicMax(&s_w[lidx], wb);
        else if (wb > weight_bits[gidx]) atomicMax(weight_bits + gidx, wb);
        if (light <= opt.stop_thresh) alive = false;
      }
      const float tn = t + delta_t;
      if (!(tn > t)) alive = false;              // step below the resolution of t: stop rather than spin
      t = tn;
      if (!(t < tmax)) alive = false;
      if (alive) next_sample();
    }
    const int n_alive = __syncthreads_count(alive ? 1 : 0);
    for (int e = tid; e < kWin * kWin * 64; e += 256) {
      const int wv = s_w[e];
      if (wv > 0) {
        const int br = e >> 6;
        const uint32_t g = ((uint32_t)k << shA) | ((uint32_t)(wb0 + br / kWin) << shB) | ((uint32_t)(wc0 + br % kWin) << shC) | (uint32_t)(e & 63);
        if (wv > weight_bits[g]) atomicMax(weight_bits + g, wv);
        s_w[e] = 0;
      }
    }
    if (n_alive == 0) return;
    // (handing the last few live rays of a tile to the per-sample path below -- fewer than 32 .. 192 of 256 -- measured
    // within 1 % on both kinds of scene: not done)
  }
  // rays still alive after the last layer of the sweep (none in practice): the per-sample path of grid_weight_kernel
  while (alive) {
    const uint32_t low = ((uint32_t)(c0 & 3) << lsA) | ((uint32_t)(c1 & 3) << lsB) | ((uint32_t)(c2 & 3) << lsC);
    const uint32_t gidx = ((uint32_t)(c0 >> 2) << shA) | ((uint32_t)(c1 >> 2) << shB) | ((uint32_t)(c2 >> 2) << shC) | low;
    const float sg = sigma[gidx];
    if (sg > opt.sigma_thresh) {
      const float att = expf(-(delta_t * delta_scale) * sg);
      const float w = light * (1.0f - att);
      light = light * att;
      const int wb = __float_as_int(w);
      if (wb > weight_bits[gidx]) atomicMax(weight_bits + gidx, wb);
      if (light <= opt.stop_thresh) break;
    }
    const float tn = t + delta_t;
    if (!(tn > t)) break;
    t = tn;
    if (!(t < tmax)) break;
    next_sample();
  }
}

template <bool BRICK, bool POW2>
__global__ __launch_bounds__(256) void grid_weight_kernel(const float* __restrict__ sigma, int reso,
                                                           const float* __restrict__ c2w_all, int n_cams, float fx, float fy,
                                                           int W, int H, PxoRenderOpts opt, Vec3 offset, Vec3 invradius,
                                                           int* __restrict__ weight_bits, PxoNdc ndc) {
  grid_weight_body<BRICK, POW2>(sigma, reso, c2w_all, n_cams, fx, fy, W, H, opt, offset, invradius, weight_bits, ndc);
}

// bricked power-of-two grids: either marcher, chosen per launch (workgroup-uniform)
__global__ __launch_bounds__(256) void grid_weight_pow2_kernel(const float* __restrict__ sigma, int reso,
                                                                const float* __restrict__ c2w_all, int n_cams, float fx, float fy,
                                                                int W, int H, PxoRenderOpts opt, Vec3 offset, Vec3 invradius,
                                                                int* __restrict__ weight_bits, GwSelect sel, PxoNdc ndc) {
  // one block of workgroup scratch for either marcher: the slab marcher's sigma / weight windows, or the per-sample marcher's
  // index tables (3 x 512 words fit the sigma window)
  constexpr int kWin = 6;
  __shared__ __attribute__((aligned(16))) float s_sigma[kWin * kWin * 64];
  __shared__ int s_w[kWin * kWin * 64];
  static_assert(kWin * kWin * 64 >= 3 * kGwLutMax, "the index tables live in the sigma window");
  if (sel.dense()) grid_weight_slab_body<kWin>(sigma, reso, c2w_all, n_cams, fx, fy, W, H, opt, offset, invradius, weight_bits, s_sigma, s_w, sel.order, ndc);
  else grid_weight_body<true, true>(sigma, reso, c2w_all, n_cams, fx, fy, W, H, opt, offset, invradius, weight_bits, ndc,
                                    reinterpret_cast<uint32_t*>(s_sigma), sel.order);
}

// ------------------------------------------------------------------------------------------
// octree renderer
// ------------------------------------------------------------------------------------------
constexpr int kRenderThreads = 256;

// lanes per ray: ROW in {4, 8, 16}; the wave carries 64/ROW rays as a WTX x WTY pixel patch (patch_wtx: the launch shape on
// the host takes the width from the same function)
__host__ __device__ constexpr int patch_wtx(int row) { return 64 / row <= 4 ? 2 : (64 / row <= 16 ? 4 : 8); }
template <int ROW> struct RowGeom {
  static constexpr int kRaysPerWave = 64 / ROW;
  static constexpr int kRaysPerBlock = kRenderThreads / ROW;
  static constexpr int kWTX = patch_wtx(ROW);
  static constexpr int kWTY = kRaysPerWave / kWTX;
  static constexpr int kMaxLoads = (75 + ROW - 1) / ROW;      // SH25: 75 coefficients
  static constexpr int kMaxGroups = (19 + ROW - 1) / ROW;     // ... as 19 groups of 4 consecutive floats
};
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a leaf row is only 4-byte aligned (49 floats)

template <int ROW>
__device__ __forceinline__ float row_sum(float v) {   // sum over the ROW lanes of a ray, result in every lane
#pragma unroll
  for (int o = 1; o < ROW; o <<= 1) v += __shfl_xor(v, o, ROW);
  return v;
}

// sh_basis_dyn / sg_basis_dyn, the per-ray basis of either tree format: pxo_sh.h (shared with pxo_shade_points)

// The argument block of the renderers of a tree with float or float16 rows (Tree: PxoTree or PxoHalfTree).  The member order
// is the kernels' kernarg layout: pinned below.
template <typename Tree>
struct FwdBlock {
  Tree tree;
  PxoCamera cam;
  int has_cam;
  const float* origins;
  const float* dirs;
  const float* viewdirs;
  int64_t B;
  PxoRenderOpts opt;
  const float* lobes;                          // NULL: SH tree; else the [basis_dim,4] lobes of an SG tree (kernel-uniform)
  PxoNdc ndc;                                  // width == 0: world-space rays; else the NDC set-up of ndc_ray (kernel-uniform)
};
using RenderArgs = FwdBlock<PxoTree>;          // also what the backward and the counting kernel take
static_assert(sizeof(RenderArgs) == 160 && offsetof(RenderArgs, opt) == 120 && offsetof(RenderArgs, lobes) == 136 &&
              offsetof(RenderArgs, ndc) == 144, "kernarg layout of the float tree's renderers");
static_assert(sizeof(FwdBlock<PxoHalfTree>) == 168 && offsetof(FwdBlock<PxoHalfTree>, opt) == 128 &&
              offsetof(FwdBlock<PxoHalfTree>, lobes) == 144 && offsetof(FwdBlock<PxoHalfTree>, ndc) == 152,
              "kernarg layout of the float16 tree's renderers");
// the per-ray basis of either tree format; everything after it sees only basis[k]
template <typename Tree>
__device__ __forceinline__ void ray_basis(const FwdBlock<Tree>& A, int basis_dim, const float (&vdir)[3], float* Y) {
  if (A.lobes) sg_basis_dyn(basis_dim, A.lobes, vdir[0], vdir[1], vdir[2], Y);
  else sh_basis_dyn(basis_dim, vdir[0], vdir[1], vdir[2], Y);
}
// what an AUX instantiation of a forward renderer takes on top: the launches without AUX keep their argument block as it is
struct AuxOut {
  float* out;                                  // [B,3]: alpha, depth, surface (plenoctree_octree.h)
  float surface_thresh;
};
template <typename Block> struct WithAux : Block, AuxOut {};
template <typename Block, bool AUX> using MaybeAux = std::conditional_t<AUX, WithAux<Block>, Block>;
// ... and a FOOT instantiation (a depth per sample from the pixel footprint; plenoctree_octree.h, "footprint")
struct FootIn {
  float foot_g;                                // fl(cone * min(invradius)): footprint per unit of world distance, in tree units
  int foot_min_depth;
};
template <typename Block> struct WithFoot : Block, FootIn {};
template <typename Block, bool FOOT> using MaybeFoot = std::conditional_t<FOOT, WithFoot<Block>, Block>;
// ST: what a leaf row stores, float (PxoTree) or _Float16 (PxoHalfTree)
template <typename ST> using TreeOf = std::conditional_t<std::is_same<ST, float>::value, PxoTree, PxoHalfTree>;

// Four consecutive halves of a float16 leaf row, widened (exactly) to float32.  ALIGN: what is known at compile time of the
// first half's index modulo 4 -- rows start 8-byte aligned (row_stride is a multiple of 4).  0: one 8-byte load; 2: two
// 4-byte loads; 1 or 3: a half, an aligned pair, a half.  No piece reads outside [p, p + 4).
typedef _Float16 f16x4a __attribute__((ext_vector_type(4), aligned(8)));
typedef _Float16 f16x2a __attribute__((ext_vector_type(2), aligned(4)));
template <int ALIGN>
__device__ __forceinline__ f32x4u load_half4(const _Float16* __restrict__ p) {
  f32x4u v;
  if constexpr (ALIGN == 0) {
    const f16x4a h = *reinterpret_cast<const f16x4a*>(p);
    v[0] = (float)h[0]; v[1] = (float)h[1]; v[2] = (float)h[2]; v[3] = (float)h[3];
  } else if constexpr (ALIGN == 2) {
    const f16x2a a = *reinterpret_cast<const f16x2a*>(p), b = *reinterpret_cast<const f16x2a*>(p + 2);
    v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)b[0]; v[3] = (float)b[1];
  } else {
    const f16x2a m = *reinterpret_cast<const f16x2a*>(p + 1);
    v[0] = (float)p[0]; v[1] = (float)m[0]; v[2] = (float)m[1]; v[3] = (float)p[3];
  }
  return v;
}

// Per-row marching state + the leaf lookup with path reuse.
struct Marcher {
  uint32_t pX, pY, pZ;
  int last_depth;
  int loads;                                   // child-pointer loads of the last find() (read by the counting kernel only)
  bool first;
  int* stack;                                  // LDS, kMaxD + 2 entries of this row

  __device__ __forceinline__ void init(int* s) {
    stack = s;
    first = true;
    last_depth = 0;
    pX = pY = pZ = 0;
    s[0] = 0;
  }
  // finds the leaf containing pos (tree coords, clamped); returns flat cell index node*8+cell
  // CAP (the footprint renderer; plenoctree_octree.h, "footprint"): the descent also stops at depth `cap` (0 <= cap <= kMaxD),
  // at a cell that may have a child, WITHOUT reading that cell's child pointer; the descent resumes no deeper than `cap`
  // either -- the previous sample may sit below it in the same cell, and its path would lead back into the fine cell.
  template <bool CAP = false>
  __device__ __forceinline__ int64_t find(const int32_t* __restrict__ child, const float (&pos)[3], int& depth_out,
                                          int cap = kMaxD) {
    const uint32_t X = (uint32_t)(pos[0] * (float)(1u << kBits));
    const uint32_t Y = (uint32_t)(pos[1] * (float)(1u << kBits));
    const uint32_t Z = (uint32_t)(pos[2] * (float)(1u << kBits));
    int depth = 0;
    if (!first) {
      const uint32_t diff = (X ^ pX) | (Y ^ pY) | (Z ^ pZ);
      const int common = diff ? (__clz((int)diff) - (32 - kBits)) : kBits;     // leading bit-levels shared
      depth = min(common, last_depth);
      if constexpr (CAP) depth = min(depth, cap);
    }
    first = false;
    pX = X; pY = Y; pZ = Z;
    int node = stack[depth];
    int cell;
    loads = 0;
    while (true) {
      const int bit = kBits - 1 - depth;
      cell = (int)(((X >> bit) & 1u) << 2 | ((Y >> bit) & 1u) << 1 | ((Z >> bit) & 1u));
      if constexpr (CAP)
        if (depth >= cap) break;                        // cap <= kMaxD: the depth bound below, and more
      const int skip = child[(int64_t)node * 8 + cell];
      ++loads;
      if (skip == 0 || (!CAP && depth >= kMaxD)) break;   // depth bound: a malformed file cannot spin the descent
      node += skip;
      ++depth;
      stack[depth] = node;
    }
    last_depth = depth;
    depth_out = depth;
    return (int64_t)node * 8 + cell;
  }
};

// One sample of a tree march: the leaf at parameter tt of ray r and the step to the next sample.  Neither depends on the
// leaf's DATA, which is what the renderers' software pipeline rests on.
// FOOT: the sample stops at the depth its pixel footprint allows (foot_cap) and steps to the exit of THAT cell; foot_k is the
// ray's footprint per unit of tt, in tree units.
__device__ __forceinline__ int foot_cap(float f, int min_depth) {
  return max(min_depth, min(126 - (int)(__float_as_uint(f) >> 23), kMaxD));      // smallest d with 2^-(d+1) <= f, clamped
}
template <bool FOOT = false>
__device__ __forceinline__ void locate_leaf(const TreeRay& r, const CellExit& cell_exit, Marcher& mk, const int32_t* child,
                                            float step_size, float tt, int64_t& leaf, float& delta, float foot_k = 0.0f,
                                            int min_depth = 0) {
  float pos[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) pos[a] = clamp_coord(r.o[a] + tt * r.d[a]);
  int depth;
  if constexpr (FOOT) leaf = mk.find<true>(child, pos, depth, foot_cap(tt * foot_k, min_depth));
  else leaf = mk.find(child, pos, depth);
  const float cube = (float)(2u << depth);
  float local[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) local[a] = __builtin_amdgcn_fractf(pos[a] * cube);
  delta = cell_exit(local) * inv_cells(depth) + step_size;
}

// Which ray row `row` of a renderer's workgroup takes, with its world-space origin, direction and view direction.  Camera
// mode: the block's 4 waves form a 2 x 2 arrangement of WTX x WTY pixel patches; explicit rays: blockIdx * kRaysPerBlock + row.
// A row past the image or the ray count is not active and leaves the three vectors untouched.  A: any renderer's argument
// block.  (ray and active come back by value: handed over by reference they would stay in memory until this function is
// inlined, and every kernel that calls it compiles to other code -- profiles/EXPERIMENTS.md.)
struct RowId { int64_t ray; bool active; };
template <int ROW, typename Args>
__device__ __forceinline__ RowId row_ray(const Args& A, int row, float (&origin)[3], float (&dir)[3], float (&vdir)[3]) {
  using G = RowGeom<ROW>;
  RowId id;
  if (A.has_cam) {
    const int W = A.cam.width, H = A.cam.height;
    const int tiles_x = (W + 2 * G::kWTX - 1) / (2 * G::kWTX);
    const int bx = (int)(blockIdx.x % tiles_x), by = (int)(blockIdx.x / tiles_x);
    const int wv = row / G::kRaysPerWave, q = row % G::kRaysPerWave;
    const int px = (bx * 2 + (wv & 1)) * G::kWTX + q % G::kWTX, py = (by * 2 + (wv >> 1)) * G::kWTY + q / G::kWTX;
    id.active = px < W && py < H;
    id.ray = (int64_t)py * W + px;
    if (id.active) {
      camera_ray(A.cam.c2w, A.cam.fx, A.cam.fy, W, H, px, py, origin, dir);
#pragma unroll
      for (int a = 0; a < 3; ++a) vdir[a] = dir[a];
    }
  } else {
    id.ray = blockIdx.x * (int64_t)G::kRaysPerBlock + row;
    id.active = id.ray < A.B;
    if (id.active) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        origin[a] = A.origins[id.ray * 3 + a];
        dir[a] = A.dirs[id.ray * 3 + a];
        vdir[a] = A.viewdirs[id.ray * 3 + a];
      }
    }
  }
  return id;
}

// MODE 0: forward (writes out_rgb).  MODE 1: gradient w.r.t. tree data (two marches per ray).
// VEC (forward only): lane l owns the float groups l, l+ROW, ... (4 consecutive data indices each) instead of the single
// indices l, l+ROW, ...: a leaf's coefficients arrive in ceil(3K/4/ROW) 16-byte loads per lane (SH16, 8 lanes: 2 instead
// of 6 dword loads).  For every SH format 3K+1 is 0 or 1 mod 4, so the last group never leaves the leaf's own row.
// KF != 0 (forward, VEC): channel-aligned ownership.  Per colour channel, lane l owns the float4 groups l, l+ROW, .. of the
// K/4 whole groups and coefficient 4 (K/4) + l of the K % 4 left over, so the basis values a lane needs are the same for
// the three channels: 4 ceil(K/4/ROW) + 1 registers instead of a selector-weighted triple per data element, and a third
// of the FMAs.  KF = K (1, 4, 9, 16, 25) makes K a compile-time constant (SH16 at 4 lanes: one float4 per lane and channel,
// 56 VGPRs - 8 waves per SIMD - against 112 for the index-ordered path); KF = -1 keeps it a run-time value (no
// forward launch instantiates that: check_format admits the five formats only; octree_render_bwd4_kernel<-1> is launched).
// AUX (forward only): three more row-uniform accumulators per ray -- alpha = sum of the weights, depth = sum of weight x
// sample distance, surface = distance of the sample at which the transmittance first falls to A.surface_thresh -- written to
// A.out[ray*3 + c] by the lanes that write out_rgb.  A sample's distance is (t + delta / 2) delta_scale with the sample's OWN
// t, kept in t_cur across the pipeline's advance of t.
// ST = _Float16 (forward, VEC): the tree is a PxoHalfTree.  A leaf row is row_stride halves, logical index i at half i; a
// coefficient and sigma are widened to float32 as they are loaded (load_half4 for the groups of four), and every lane owns
// the logical indices, multiplies and adds in the order of the float instantiation with the same MODE, ROW, KF and AUX: the
// two return the same bits for a tree whose float data is the widened halves.
// FOOT (forward, float rows): every sample stops its descent at the depth its pixel footprint allows and reads the row there,
// the filled row of pxo_tree_lod_fill where the cell has a child (locate_leaf<true>).  One register per ray (foot_k); per
// sample a multiply, a shift, a subtract and a clamp.  Nothing else in the kernel knows of it.
template <int MODE, int ROW, bool VEC = false, int KF = 0, bool AUX = false, typename ST = float, bool FOOT = false>
__global__ __launch_bounds__(kRenderThreads) void octree_render_kernel(MaybeFoot<MaybeAux<FwdBlock<TreeOf<ST>>, AUX>, FOOT> A,
                                                                        float* __restrict__ out_rgb,
                                                                        const float* __restrict__ fwd_rgb,
                                                                        const float* __restrict__ grad_out,
                                                                        float* __restrict__ grad_data) {
  using G = RowGeom<ROW>;
  constexpr int kRow = ROW, kRaysPerBlock = G::kRaysPerBlock, kMaxLoads = G::kMaxLoads;
  __shared__ int s_stack[kRaysPerBlock][kMaxD + 2];
  __shared__ float s_basis[kRaysPerBlock][25];
  const int row = threadIdx.x / kRow, l = threadIdx.x % kRow;
  float origin[3], dir[3], vdir[3];
  const RowId id = row_ray<ROW>(A, row, origin, dir, vdir);
  if (!id.active) return;                      // whole rows leave together; no block-level barrier below
  const int64_t ray = id.ray;

  const int K = A.tree.basis_dim, D = A.tree.data_dim;
  const float bg = A.opt.background_brightness;
  bool ndc_miss = false;
  if constexpr (!AUX)                          // the extra outputs are world-space distances: no NDC form of them
    if (A.ndc.width > 0) ndc_miss = !ndc_ray(A.ndc, origin, dir);        // vdir stays the world-space direction
  TreeRay r;
  to_tree_ray(origin, dir, A.tree.offset, A.tree.invradius, r);
  CellExit cell_exit;
  cell_exit.init(r.invdir);
  const bool miss = ndc_miss || r.tmax < 0.0f || r.tmin > r.tmax;
  static_assert(!AUX || MODE == 0, "alpha / depth / surface: forward only");
  static_assert(!FOOT || (MODE == 0 && std::is_same_v<ST, float>), "footprint depth: forward, float rows");
  float foot_k = 0.0f;
  int foot_min = 0;
  if constexpr (FOOT) {
    foot_k = r.delta_scale * A.foot_g;
    foot_min = A.foot_min_depth;
  }
  if (MODE == 0 && miss) {
    for (int c = l; c < 3; c += kRow) out_rgb[ray * 3 + c] = bg;
    if constexpr (AUX)
      for (int c = l; c < 3; c += kRow) A.out[ray * 3 + c] = c == 2 ? INFINITY : 0.0f;
    return;
  }
  if (MODE == 1 && miss) return;

  // per-lane channel ownership: data index l + ROW j -> (channel, SH component)
  if (l == 0) ray_basis(A, K, vdir, s_basis[row]);
  __builtin_amdgcn_wave_barrier();
  static_assert(!VEC || MODE == 0, "vector loads: forward only (the gradient scatter wants contiguous dword rows)");
  static_assert(KF == 0 || (VEC && MODE == 0), "channel-aligned paths: forward, vector loads");
  constexpr bool HALF = std::is_same_v<ST, _Float16>;
  static_assert(std::is_same_v<ST, float> || (HALF && VEC && MODE == 0 && KF >= 0), "float16 rows: forward, vector loads, K known");
  const int Kc = KF > 0 ? KF : K;                    // compile-time when the launch is specialised for the tree's format
  constexpr int kChM = ((KF > 0 ? KF / 4 : 6) + ROW - 1) / ROW > 0 ? ((KF > 0 ? KF / 4 : 6) + ROW - 1) / ROW : 1;   // K <= 25: <= 6 whole groups
  const int chG = Kc >> 2, chR = Kc & 3;
  float bk[4 * kChM], bk_r = 0.0f;
  if (KF != 0) {
#pragma unroll
    for (int m = 0; m < kChM; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) bk[4 * m + e] = (l + kRow * m) < chG ? s_basis[row][4 * (l + kRow * m) + e] : 0.0f;
    if (l < chR) bk_r = s_basis[row][4 * chG + l];
  }
  constexpr int kSlots = KF ? 1 : (VEC ? G::kMaxGroups * 4 : kMaxLoads);       // data elements owned by a lane (generic paths)
  const int nload = VEC ? ((D - 1 + 3) / 4 + kRow - 1) / kRow : (D - 1 + kRow - 1) / kRow;   // loads per lane in use
  float b0[kSlots], b1[kSlots], b2[kSlots];
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int idx = VEC ? 4 * (l + kRow * (j >> 2)) + (j & 3) : l + kRow * j;
    float bas = 0.0f;
    int ch = -1;
    if (KF == 0 && (VEC ? (j >> 2) : j) < nload && idx < D - 1) {
      ch = idx / K;
      bas = s_basis[row][idx - ch * K];
    }
    b0[j] = ch == 0 ? bas : 0.0f;
    b1[j] = ch == 1 ? bas : 0.0f;
    b2[j] = ch == 2 ? bas : 0.0f;
  }
  const ST* __restrict__ data = static_cast<const ST*>(A.tree.data);
  const int32_t* __restrict__ child = A.tree.child;
  int row_elems = D;                           // from a leaf's row to the next, in elements of ST
  if constexpr (HALF) row_elems = A.tree.row_stride;

  float g[3] = {0.f, 0.f, 0.f};
  if (MODE == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = grad_out[ray * 3 + c];
  }
  float accum = 0.0f;                          // MODE 1: sum_c g_c * out_c, then the part behind the sample
  int first_pass = 0;
  if (MODE == 1 && fwd_rgb != nullptr) {       // the caller kept the (exact) forward image: no first march
    accum = (g[0] * fwd_rgb[ray * 3] + g[1] * fwd_rgb[ray * 3 + 1]) + g[2] * fwd_rgb[ray * 3 + 2];
    first_pass = 1;
  }

  // pass 0 composites; in MODE 1 pass 1 re-marches and scatters the gradient
  for (int pass = first_pass; pass <= MODE; ++pass) {
    Marcher mk;
    mk.init(s_stack[row]);
    float t = r.tmin, light = 1.0f;
    float out[3] = {0.f, 0.f, 0.f};
    float aux[3] = {0.f, 0.f, INFINITY};         // AUX: alpha, depth, surface
    bool stopped = false;
    // locate_leaf does not depend on the leaf's DATA.  The march is software-pipelined on that: a sample's sigma is requested, then the NEXT sample is located (its child-pointer loads
    // travel together with the sigma request), and only then is the current sample shaded -- per sample one dependent L2 round
    // trip less (lookup || sigma -> coefficients instead of lookup -> sigma -> coefficients).  Same samples, same arithmetic.
    auto locate = [&](float tt, int64_t& leaf_o, float& delta_o) {
      locate_leaf<FOOT>(r, cell_exit, mk, child, A.opt.step_size, tt, leaf_o, delta_o, foot_k, foot_min);
    };
    int64_t leaf = 0;
    float delta_t = 0.0f;
    bool more = t < r.tmax;
    if (more) locate(t, leaf, delta_t);
    while (more) {
      const ST* __restrict__ val = data + leaf * row_elems;
      const float sg = (float)val[D - 1];
      const float tn = t + delta_t;
      more = tn > t && tn < r.tmax;           // !(tn > t): step below the resolution of t, stop rather than spin
      const int64_t leaf_cur = leaf;
      const float delta_cur = delta_t;
      const float t_cur = t;
      if (more) locate(tn, leaf, delta_t);       // the next sample, while sigma is on its way
      t = tn;
      if (sg > A.opt.sigma_thresh) {
        const float dtw = delta_cur * r.delta_scale;
        const float att = expf(-dtw * sg);
        const float weight = light * (1.0f - att);
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        if (KF != 0) {
#pragma unroll
          for (int m = 0; m < kChM; ++m) {
            const int g = l + kRow * m;
            if (g < chG) {
              f32x4u c0, c1, c2;
              if constexpr (HALF) {                // channel c starts at half c K: its alignment is that of c KF modulo 4
                c0 = load_half4<0>(val + 4 * g);
                c1 = load_half4<KF % 4>(val + Kc + 4 * g);
                c2 = load_half4<2 * KF % 4>(val + 2 * Kc + 4 * g);
              } else {
                c0 = *reinterpret_cast<const f32x4u*>(val + 4 * g);
                c1 = *reinterpret_cast<const f32x4u*>(val + Kc + 4 * g);
                c2 = *reinterpret_cast<const f32x4u*>(val + 2 * Kc + 4 * g);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                p0 += c0[e] * bk[4 * m + e];
                p1 += c1[e] * bk[4 * m + e];
                p2 += c2[e] * bk[4 * m + e];
              }
            }
          }
          if (l < chR) {
            const int k = 4 * chG + l;
            p0 += (float)val[k] * bk_r;
            p1 += (float)val[Kc + k] * bk_r;
            p2 += (float)val[2 * Kc + k] * bk_r;
          }
        } else if (VEC) {
#pragma unroll
          for (int j = 0; j < G::kMaxGroups; ++j) {
            const int g4 = 4 * (l + kRow * j);
            if (j < nload && g4 < D - 1) {
              f32x4u v4;
              if constexpr (HALF) v4 = load_half4<0>(val + g4);         // g4 + 3 < row_stride: inside the row's padding at most
              else v4 = *reinterpret_cast<const f32x4u*>(val + g4);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float v = g4 + e < D - 1 ? v4[e] : 0.0f;         // the row's last float is sigma, not a coefficient
                p0 += v * b0[4 * j + e];
                p1 += v * b1[4 * j + e];
                p2 += v * b2[4 * j + e];
              }
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < kMaxLoads; ++j) {
            if (j < nload) {
              const int idx = l + kRow * j;
              const float v = idx < D - 1 ? (float)val[idx] : 0.0f;
              p0 += v * b0[j];
              p1 += v * b1[j];
              p2 += v * b2[j];
            }
          }
        }
        p0 = row_sum<ROW>(p0);
        p1 = row_sum<ROW>(p1);
        p2 = row_sum<ROW>(p2);
        const float c0 = 1.0f / (1.0f + expf(-p0)), c1 = 1.0f / (1.0f + expf(-p1)), c2 = 1.0f / (1.0f + expf(-p2));
        if (pass == 0) {
          out[0] += weight * c0;
          out[1] += weight * c1;
          out[2] += weight * c2;
          light = light * att;
          if constexpr (AUX) {
            const float s = (t_cur + 0.5f * delta_cur) * r.delta_scale;
            aux[0] += weight;
            aux[1] += weight * s;
            if (light <= A.surface_thresh && aux[2] == INFINITY) aux[2] = s;
          }
          if (MODE == 0 && light <= A.opt.stop_thresh) {
            const float scale = 1.0f / (1.0f - light);
            out[0] *= scale; out[1] *= scale; out[2] *= scale;
            if constexpr (AUX) { aux[0] *= scale; aux[1] *= scale; }
            stopped = true;
            break;
          }
        } else {
          const float total = (g[0] * c0 + g[1] * c1) + g[2] * c2;
          const float d0 = weight * g[0] * c0 * (1.0f - c0);
          const float d1 = weight * g[1] * c1 * (1.0f - c1);
          const float d2 = weight * g[2] * c2 * (1.0f - c2);
          float* __restrict__ gv = grad_data + leaf_cur * D;
#pragma unroll
          for (int j = 0; j < kMaxLoads; ++j) {
            if (j < nload) {
              const int idx = l + kRow * j;
              if (idx < D - 1) unsafeAtomicAdd(gv + idx, (b0[j] * d0 + b1[j] * d1) + b2[j] * d2);
            }
          }
          light = light * att;
          accum -= weight * total;
          if (l == 0) unsafeAtomicAdd(gv + D - 1, dtw * (total * light - accum));
        }
      }
    }
    if (pass == 0) {
      if (MODE == 0) {
        if (!stopped) {
          out[0] += light * bg; out[1] += light * bg; out[2] += light * bg;
        }
        for (int c = l; c < 3; c += kRow) out_rgb[ray * 3 + c] = c == 0 ? out[0] : (c == 1 ? out[1] : out[2]);
        if constexpr (AUX)
          for (int c = l; c < 3; c += kRow) A.out[ray * 3 + c] = c == 0 ? aux[0] : (c == 1 ? aux[1] : aux[2]);
      } else {
        accum = (g[0] * (out[0] + light * bg) + g[1] * (out[1] + light * bg)) + g[2] * (out[2] + light * bg);
      }
    }
  }
}

// Backward with a 4-lane march and a 16-lane scatter.  The march is the forward kernel's: 16 rays per wave,
// channel-aligned coefficient reads, few registers - the phase that is latency-bound.  The scatter wants the opposite shape
// (the gradient of a sample is a 3K-float row: 64-byte atomic rows per instruction), so after every march step the wave
// re-deals itself as 4 rays x 16 lanes, four times: lane (q, j) of deal g fetches the step's row-uniform results of ray
// 4g + q from that ray's lanes (shfl) and adds basis_k(ray) * d_channel at the data indices j, j + 16, .. - the same 64-byte rows per
// instruction as the 16-lane kernel, with the march running at four times its rays per wave.  Rays that have finished stay in
// the loop (idle) until the whole wave is done, since every lane takes part in every deal.
// UPD (WC > 0): how a sample's gradient row reaches the wave's cache.
//   0  one sample at a time, the whole wave on its 3K+1-float row (15 of 64 lanes idle for SH16, ~27 vector instructions per
//      sample, ~12 samples per march step of the wave's 16 rays: the update phase issued twice the instructions of the march);
//   1  every ray's own 4 lanes add its sample's row -- 13 (SH16) / 19 (SH25) LDS float atomics per lane, all 16 rays at once --
//      when the slot already holds the ray's leaf (a hit); rays that miss elect ONE winner per slot through LDS, the winners' old
//      rows leave as before (one contiguous row of global atomics per row, the whole wave on it) and the winners write their new
//      rows themselves; rays that lost an election go round again and usually hit the row the winner has just installed (the
//      neighbouring pixel entered the same leaf in the same step).  A wave's LDS operations execute in program order, so the
//      hits of a round land before the evictions read the rows and the installs after.  Measured (r05c): 4.27 / 4.28 ms against
//      4.26 / 4.29 ms for form 0 -- no gain (the kernel is bound by its evicted rows, not by issue): form 0 stays the default.
template <int KF, int WC, int UPD = 0>
__global__ __launch_bounds__(kRenderThreads) void octree_render_bwd4_kernel(RenderArgs A, const float* __restrict__ fwd_rgb,
                                                                             const float* __restrict__ grad_out,
                                                                             float* __restrict__ grad_data) {
  using G = RowGeom<4>;
  constexpr int kRow = 4, kRaysPerBlock = G::kRaysPerBlock;
  constexpr int kDmax = 3 * (KF > 0 ? KF : 25) + 1, kRM = (kDmax + 63) / 64, kWCn = WC > 0 ? WC : 1;
  constexpr int kPM = (kDmax + kRow - 1) / kRow;                 // row elements per lane of a ray (UPD 1): l, l + 4, ...
  __shared__ int s_stack[kRaysPerBlock][kMaxD + 2];
  __shared__ float s_basis[kRaysPerBlock][25];
  __shared__ float s_rows[kRenderThreads / 64][kWCn][WC > 0 ? kDmax : 1];
  __shared__ int s_tag[kRenderThreads / 64][UPD ? kWCn : 1];     // UPD 1: the leaf whose row sits in slot i (-1: empty)
  __shared__ int s_own[kRenderThreads / 64][UPD ? kWCn : 1];     //        the ray that won the slot in this round
  static_assert(WC <= 64, "one tag per lane");
  static_assert(UPD == 0 || WC > 0, "the ray-parallel update needs the cache");
  const int row = threadIdx.x / kRow, l = threadIdx.x % kRow, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int tagv = -1;                                 // lane i: the leaf whose row sits in slot i of this wave's cache (-1: empty)
  float origin[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 1.f}, vdir[3] = {0.f, 0.f, 1.f};
  const RowId id = row_ray<kRow>(A, row, origin, dir, vdir);            // an inactive row keeps the finite ray above
  const int64_t ray = id.ray;
  bool active = id.active;
  const int K = A.tree.basis_dim, D = A.tree.data_dim;
  const int Kc = KF > 0 ? KF : K;
  const float bg = A.opt.background_brightness;
  if (A.ndc.width > 0) active = ndc_ray(A.ndc, origin, dir) && active;   // an NDC miss: no march, no gradient
  TreeRay r;
  to_tree_ray(origin, dir, A.tree.offset, A.tree.invradius, r);
  CellExit cell_exit;
  cell_exit.init(r.invdir);
  const bool alive = active && !(r.tmax < 0.0f || r.tmin > r.tmax);

  if (l == 0) {
    if (alive) ray_basis(A, K, vdir, s_basis[row]);
    else
      for (int i = 0; i < 25; ++i) s_basis[row][i] = 0.0f;
  }
  __builtin_amdgcn_wave_barrier();
  // march side: channel-aligned ownership (see octree_render_kernel, KF)
  constexpr int kChM = ((KF > 0 ? KF / 4 : 6) + kRow - 1) / kRow > 0 ? ((KF > 0 ? KF / 4 : 6) + kRow - 1) / kRow : 1;
  const int chG = Kc >> 2, chR = Kc & 3;
  float bk[4 * kChM], bk_r = 0.0f;
#pragma unroll
  for (int m = 0; m < kChM; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) bk[4 * m + e] = (l + kRow * m) < chG ? s_basis[row][4 * (l + kRow * m) + e] : 0.0f;
  if (l < chR) bk_r = s_basis[row][4 * chG + l];
  // scatter side: in deal g this lane serves ray 4 g + (lane >> 4) of the wave, data indices j, j + 16, .. of the leaf row
  // (index-ordered, so every instruction adds 64 contiguous bytes per ray whatever K is)
  constexpr int kSM = (3 * (KF > 0 ? KF : 25) + 15) / 16;
  const int j = lane & 15, wave_row0 = (row / G::kRaysPerWave) * G::kRaysPerWave;
  float sb[4][kSM];
  int sch[kSM];
#pragma unroll
  for (int m = 0; m < kSM; ++m) {
    const int idx = j + 16 * m;
    sch[m] = idx < 3 * Kc ? idx / Kc : -1;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      sb[gq][m] = sch[m] >= 0 ? s_basis[wave_row0 + 4 * gq + (lane >> 4)][idx - sch[m] * Kc] : 0.0f;
  }
  // write-combining side: the wave's lane owns the data indices lane, lane + 64 of whatever row is being updated
  int wch[kRM], wof[kRM];
#pragma unroll
  for (int m = 0; m < kRM; ++m) {
    const int idx = lane + 64 * m;
    wch[m] = idx < 3 * Kc ? idx / Kc : 3;
    wof[m] = idx < 3 * Kc ? idx - wch[m] * Kc : 0;
  }
  // ray-parallel side (UPD 1): this lane owns the data indices l, l + 4, .. of its OWN ray's sample row: basis value and channel
  // (3 = the sigma entry, 4 = past the row) per owned index
  float pb[UPD ? kPM : 1];
  int pch[UPD ? kPM : 1];
  if (UPD) {
#pragma unroll
    for (int m = 0; m < kPM; ++m) {
      const int idx = l + kRow * m;
      pch[m] = idx < 3 * Kc ? idx / Kc : (idx == D - 1 ? 3 : 4);
      pb[m] = idx < 3 * Kc ? s_basis[row][idx - pch[m] * Kc] : (idx == D - 1 ? 1.0f : 0.0f);
    }
    if (lane < kWCn) s_tag[wave][lane] = -1;
  }
  const int ray_in_wave = lane >> 2;
  const float* __restrict__ data = A.tree.data;
  const int32_t* __restrict__ child = A.tree.child;

  float g[3] = {0.f, 0.f, 0.f};
  if (alive) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = grad_out[ray * 3 + c];
  }
  float accum = 0.0f;
  int first_pass = 0;
  if (fwd_rgb != nullptr) {                    // the caller kept the (exact) forward image: no first march
    if (alive) accum = (g[0] * fwd_rgb[ray * 3] + g[1] * fwd_rgb[ray * 3 + 1]) + g[2] * fwd_rgb[ray * 3 + 2];
    first_pass = 1;
  }
  for (int pass = first_pass; pass <= 1; ++pass) {
    Marcher mk;
    mk.init(s_stack[row]);
    float t = r.tmin, light = 1.0f;
    float out[3] = {0.f, 0.f, 0.f};
    bool running = alive && t < r.tmax;
    while (__builtin_amdgcn_ballot_w64(running) != 0) {
      bool has = false;
      int leaf_i = 0;
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, es = 0.f;
      if (running) {
        int64_t leaf;
        float delta_t;
        locate_leaf(r, cell_exit, mk, child, A.opt.step_size, t, leaf, delta_t);
        const float* __restrict__ val = data + leaf * D;
        const float sg = val[D - 1];
        if (sg > A.opt.sigma_thresh) {
          const float dtw = delta_t * r.delta_scale;
          const float att = expf(-dtw * sg);
          const float weight = light * (1.0f - att);
          float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
          for (int m = 0; m < kChM; ++m) {
            const int gi = l + kRow * m;
            if (gi < chG) {
              const f32x4u c0 = *reinterpret_cast<const f32x4u*>(val + 4 * gi);
              const f32x4u c1 = *reinterpret_cast<const f32x4u*>(val + Kc + 4 * gi);
              const f32x4u c2 = *reinterpret_cast<const f32x4u*>(val + 2 * Kc + 4 * gi);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                p0 += c0[e] * bk[4 * m + e];
                p1 += c1[e] * bk[4 * m + e];
                p2 += c2[e] * bk[4 * m + e];
              }
            }
          }
          if (l < chR) {
            const int k = 4 * chG + l;
            p0 += val[k] * bk_r;
            p1 += val[Kc + k] * bk_r;
            p2 += val[2 * Kc + k] * bk_r;
          }
          p0 = row_sum<kRow>(p0);
          p1 = row_sum<kRow>(p1);
          p2 = row_sum<kRow>(p2);
          const float c0 = 1.0f / (1.0f + expf(-p0)), c1 = 1.0f / (1.0f + expf(-p1)), c2 = 1.0f / (1.0f + expf(-p2));
          if (pass == 0) {
            out[0] += weight * c0;
            out[1] += weight * c1;
            out[2] += weight * c2;
            light = light * att;
          } else {
            const float total = (g[0] * c0 + g[1] * c1) + g[2] * c2;
            e0 = weight * g[0] * c0 * (1.0f - c0);
            e1 = weight * g[1] * c1 * (1.0f - c1);
            e2 = weight * g[2] * c2 * (1.0f - c2);
            light = light * att;
            accum -= weight * total;
            es = dtw * (total * light - accum);
            leaf_i = (int)leaf;                    // n_internal < 2^28: node * 8 + cell fits 31 bits
            has = true;
          }
        }
        const float tn = t + delta_t;
        running = tn > t && tn < r.tmax;           // !(tn > t): step below the resolution of t, stop rather than spin
        t = tn;
      }
      if (pass == 1 && WC > 0 && UPD == 1) {
        float vv[kPM];
#pragma unroll
        for (int m = 0; m < kPM; ++m)
          vv[m] = pb[m] * (pch[m] == 0 ? e0 : (pch[m] == 1 ? e1 : (pch[m] == 2 ? e2 : es)));
        const int slot = (int)(((uint32_t)leaf_i * 2654435761u) >> 16) & (kWCn - 1);
        float* const rowp = s_rows[wave][slot] + l;
        bool pend = has;
        while (__builtin_amdgcn_ballot_w64(pend) != 0) {
          const int tag = pend ? s_tag[wave][slot] : -2;
          if (pend && tag == leaf_i) {                          // hit: this ray's 4 lanes add its row
#pragma unroll
            for (int m = 0; m < kPM; ++m)
              if (pch[m] < 4) __hip_atomic_fetch_add(rowp + kRow * m, vv[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            pend = false;
          }
          if (pend && l == 0) s_own[wave][slot] = ray_in_wave;   // the rays that missed: one winner per slot
          const bool win = pend && s_own[wave][slot] == ray_in_wave;
          // the winners' old rows leave, each as ONE contiguous row of atomics with the whole wave on it
          uint64_t em = __builtin_amdgcn_ballot_w64(win && l == 0 && tag >= 0);
          while (em) {
            const int src = __builtin_ctzll(em);
            em &= em - 1;
            const int sl = __builtin_amdgcn_readlane(slot, src);
            const int tg = __builtin_amdgcn_readlane(tag, src);
            const float* rp = s_rows[wave][sl];
#pragma unroll
            for (int m = 0; m < kRM; ++m) {
              const int idx = lane + 64 * m;
              if (idx < D) unsafeAtomicAdd(grad_data + (int64_t)tg * D + idx, rp[idx]);
            }
          }
          if (win) {                                            // ... and the winners start their new rows
#pragma unroll
            for (int m = 0; m < kPM; ++m)
              if (pch[m] < 4) rowp[kRow * m] = vv[m];
            if (l == 0) s_tag[wave][slot] = leaf_i;
            pend = false;
          }
        }
      }
      if (pass == 1 && WC > 0 && UPD == 0) {
        // one sample at a time, the whole wave on its row: hit -> add in LDS; miss -> the evicted row leaves as ONE
        // contiguous row of atomics, the new row starts from this sample
        uint64_t hm = __builtin_amdgcn_ballot_w64(has && l == 0);
        while (hm) {
          const int src = __builtin_ctzll(hm);
          hm &= hm - 1;
          const int lf = __builtin_amdgcn_readlane(leaf_i, src);
          const float q0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e0), src));
          const float q1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e1), src));
          const float q2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2), src));
          const float qs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(es), src));
          const int slot = (int)(((uint32_t)lf * 2654435761u) >> 16) & (kWCn - 1);
          const int tag = __builtin_amdgcn_readlane(tagv, slot);
          float* rowp = s_rows[wave][slot];
          const float* bas = s_basis[wave_row0 + (src >> 2)];
#pragma unroll
          for (int m = 0; m < kRM; ++m) {
            const int idx = lane + 64 * m;
            if (idx < D) {
              const float v = wch[m] < 3 ? bas[wof[m]] * (wch[m] == 0 ? q0 : (wch[m] == 1 ? q1 : q2)) : qs;
              if (tag == lf) {
                rowp[idx] += v;          // (as ds_add_f32, one LDS instruction instead of read-add-write: measured 1.9 % SLOWER,
                                         //  4.82 vs 4.73 ms per image, round 4: the LDS atomic unit is the slower path)
              } else {
                if (tag >= 0) unsafeAtomicAdd(grad_data + (int64_t)tag * D + idx, rowp[idx]);
                rowp[idx] = v;
              }
            }
          }
          tagv = lane == slot ? lf : tagv;
        }
      }
      if (pass == 1 && WC == 0) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int src = 4 * (4 * gq + (lane >> 4));            // first lane of the served ray's row
          const int h = __shfl((int)has, src);
          if (__builtin_amdgcn_ballot_w64(h != 0) == 0) continue;   // no sample in this deal (wave-uniform)
          const int lf = __shfl(leaf_i, src);
          const float q0 = __shfl(e0, src), q1 = __shfl(e1, src), q2 = __shfl(e2, src), qs = __shfl(es, src);
          if (h) {
            float* __restrict__ gv = grad_data + (int64_t)lf * D;
#pragma unroll
            for (int m = 0; m < kSM; ++m)
              if (sch[m] >= 0)
                unsafeAtomicAdd(gv + j + 16 * m, sb[gq][m] * (sch[m] == 0 ? q0 : (sch[m] == 1 ? q1 : q2)));
            if (j == 0) unsafeAtomicAdd(gv + D - 1, qs);
          }
        }
      }
    }
    if (pass == 0) accum = (g[0] * (out[0] + light * bg) + g[1] * (out[1] + light * bg)) + g[2] * (out[2] + light * bg);
  }
  if (WC > 0) {                                  // rows still held by the wave
    for (int sl = 0; sl < WC; ++sl) {
      const int tag = UPD ? __builtin_amdgcn_readfirstlane(s_tag[wave][sl]) : __builtin_amdgcn_readlane(tagv, sl);
      if (tag < 0) continue;
#pragma unroll
      for (int m = 0; m < kRM; ++m) {
        const int idx = lane + 64 * m;
        if (idx < D) unsafeAtomicAdd(grad_data + (int64_t)tag * D + idx, s_rows[wave][sl][idx]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// work counters (roofline pass, scripts/octree_bench.py): the marchers' own ray set-up, leaf lookup, step rule and
// early stop -- same arithmetic, so the same sample sequence -- counting instead of shading.  One thread per ray.
//   counts[0] rays that enter the volume      counts[2] samples above sigma_thresh (one full row / one weight update each)
//   counts[1] samples (one sigma read each)   counts[3] child-pointer loads of the leaf lookups (tree marcher only)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void flush_counts(unsigned long long (&c)[4], unsigned long long* __restrict__ counts) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned long long v = c[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(counts + i, v);
  }
}

__global__ __launch_bounds__(256) void octree_count_kernel(RenderArgs A, unsigned long long* __restrict__ counts,
                                                           uint8_t* __restrict__ leaf_seen) {
  __shared__ int s_stack[256][kMaxD + 2];
  unsigned long long c[4] = {0, 0, 0, 0};
  const int W = A.cam.width, H = A.cam.height;
  const int64_t ray = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (ray < (int64_t)W * H) {
    float origin[3], dir[3];
    camera_ray(A.cam.c2w, A.cam.fx, A.cam.fy, W, H, (int)(ray % W), (int)(ray / W), origin, dir);
    TreeRay r;
    to_tree_ray(origin, dir, A.tree.offset, A.tree.invradius, r);
    CellExit cell_exit;
    cell_exit.init(r.invdir);
    if (!(r.tmax < 0.0f || r.tmin > r.tmax)) {
      c[0] = 1;
      const int D = A.tree.data_dim;
      const float* __restrict__ data = A.tree.data;
      const int32_t* __restrict__ child = A.tree.child;
      Marcher mk;
      mk.init(s_stack[threadIdx.x]);
      float t = r.tmin, light = 1.0f;
      while (t < r.tmax) {
        int64_t leaf;
        float delta_t;
        locate_leaf(r, cell_exit, mk, child, A.opt.step_size, t, leaf, delta_t);
        c[3] += (unsigned long long)mk.loads;
        const float sg = data[leaf * D + D - 1];
        c[1] += 1;
        if (sg > A.opt.sigma_thresh) {
          c[2] += 1;
          if (leaf_seen) leaf_seen[leaf] = 1;
          light = light * expf(-(delta_t * r.delta_scale) * sg);
          if (light <= A.opt.stop_thresh) break;
        }
        const float tn = t + delta_t;
        if (!(tn > t)) break;
        t = tn;
      }
    }
  }
  flush_counts(c, counts);
}

__global__ __launch_bounds__(256) void grid_count_kernel(const float* __restrict__ sigma, int reso, const float* __restrict__ c2w_all,
                                                         int n_cams, float fx, float fy, int W, int H, PxoRenderOpts opt,
                                                         Vec3 offset, Vec3 invradius, unsigned long long* __restrict__ counts,
                                                         uint8_t* __restrict__ voxel_seen) {
  unsigned long long c[4] = {0, 0, 0, 0};
  const int64_t id = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int64_t hw = (int64_t)W * H;
  if (id < hw * n_cams) {
    const int cam = (int)(id / hw);
    const int64_t pix = id % hw;
    float origin[3], dir[3];
    camera_ray(c2w_all + (int64_t)cam * 12, fx, fy, W, H, (int)(pix % W), (int)(pix / W), origin, dir);
    TreeRay r;
    to_tree_ray(origin, dir, offset.v, invradius.v, r);
    if (!(r.tmax < 0.0f || r.tmin > r.tmax)) {
      c[0] = 1;
      const float cube = (float)reso;
      CellExit cell_exit;
      cell_exit.init(r.invdir);
      float t = r.tmin, light = 1.0f;
      while (t < r.tmax) {
        float local[3];
        int cc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float p = clamp_coord(r.o[a] + t * r.d[a]) * cube;
          cc[a] = (int)p;
          local[a] = __builtin_amdgcn_fractf(p);
        }
        const float delta_t = cell_exit(local) / cube + opt.step_size;     // reso a power of two: the exact quotient either way
        const int64_t idx = ((int64_t)cc[0] * reso + cc[1]) * reso + cc[2];
        const float sg = sigma[idx];
        c[1] += 1;
        if (sg > opt.sigma_thresh) {
          c[2] += 1;
          if (voxel_seen) voxel_seen[idx] = 1;
          light = light * expf(-(delta_t * r.delta_scale) * sg);
          if (light <= opt.stop_thresh) break;
        }
        const float tn = t + delta_t;
        if (!(tn > t)) break;
        t = tn;
      }
    }
  }
  flush_counts(c, counts);
}

// ------------------------------------------------------------------------------------------
// image loss and SGD
// ------------------------------------------------------------------------------------------
constexpr int kMseBlock = 256;          // threads of a workgroup of image_mse_kernel
constexpr int kMsePerThread = 8;        // elements per thread the launcher sizes the grid for ...
constexpr int kMseMaxBlocks = 4096;     // ... up to this many workgroups; a larger image takes more grid-stride iterations

__global__ __launch_bounds__(kMseBlock) void image_mse_kernel(const float* __restrict__ im, const float* __restrict__ gt, int64_t n,
                                                         float* __restrict__ grad, float* __restrict__ sse) {
  __shared__ float s_part[4];
  float acc = 0.0f;
  const float scale = 2.0f / (float)n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = im[i];
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);      // comparisons, not fmaxf / fminf: a NaN pixel stays NaN, as torch.clamp keeps it
    const float e = c - gt[i];
    acc += e * e;
    if (grad) grad[i] = (v >= 0.0f && v <= 1.0f) ? scale * e : 0.0f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sse, (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n, float lr,
                           float mu, int nesterov, int first) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gi = g[i];
  if (mu != 0.0f) {
    const float b = first ? gi : mu * buf[i] + gi;
    buf[i] = b;
    gi = nesterov ? gi + mu * b : b;
  }
  p[i] = p[i] - lr * gi;
}

// ------------------------------------------------------------------------------------------
// palette-form renderer: compressed trees (octree/compression.py:88-139) read in place, forward only.
// Device layout: include/plenoctree_octree.h (PxoQuantLayout).
// ------------------------------------------------------------------------------------------
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));        // a palette entry / a retained plane: (r, g, b, 0), 8 bytes
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));        // four consecutive palette indices of a leaf, 8 bytes

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// one thread per (group of four planes, cell), cells fastest: the 2-byte reads of a wave are one contiguous run of a plane
__global__ void quant_pack_idx_kernel(const uint16_t* __restrict__ qmap, int64_t cells, int Kq, int groups,
                                      u16x4* __restrict__ idx) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= cells * groups) return;
  const int64_t cell = i % cells;
  const int g = (int)(i / cells);
  u16x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = 4 * g + e;
    v[e] = q < Kq ? qmap[(int64_t)q * cells + cell] : (uint16_t)0;
  }
  idx[cell * groups + g] = v;
}

// [m, 3] float16 -> [m, 4]: palette entries (m = Kq * 2^bits)
__global__ void quant_pack_pad_kernel(const _Float16* __restrict__ src, int64_t m, f16x4* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  f16x4 v;
  v[0] = src[i * 3]; v[1] = src[i * 3 + 1]; v[2] = src[i * 3 + 2]; v[3] = (_Float16)0.0f;
  dst[i] = v;
}

// data_retained [r, cells, 3] float16 -> [cells, r, 4]
__global__ void quant_pack_retained_kernel(const _Float16* __restrict__ src, int64_t cells, int r, f16x4* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;       // (plane, cell), cells fastest
  if (i >= cells * r) return;
  const int64_t cell = i % cells;
  const int b = (int)(i / cells);
  f16x4 v;
  v[0] = src[i * 3]; v[1] = src[i * 3 + 1]; v[2] = src[i * 3 + 2]; v[3] = (_Float16)0.0f;
  dst[cell * r + b] = v;
}

template <typename T>
__global__ void quant_pack_sigma_kernel(const T* __restrict__ src, int64_t cells, float* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < cells) dst[i] = (float)src[i];
}

// float16 trees (PxoHalfTree): the file's [cells, D] rows at a stride of row_stride halves, zeros in the padding.  One thread
// per packed half.
__global__ void half_pack_kernel(const _Float16* __restrict__ src, int64_t cells, int D, int row_stride,
                                 _Float16* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= cells * row_stride) return;
  const int64_t r = i / row_stride;
  const int e = (int)(i - r * row_stride);
  dst[i] = e < D ? src[r * D + e] : (_Float16)0.0f;
}

struct QuantRenderArgs {
  PxoQuantTree tree;
  PxoCamera cam;
  int has_cam;
  const float* origins;
  const float* dirs;
  const float* viewdirs;
  int64_t B;
  PxoRenderOpts opt;
};

// octree_render_kernel<0, ROW>'s rays, march and compositing; a shaded sample's colour comes through the palettes.  Plane
// ownership inside a ray's ROW lanes: lane l owns the retained planes l, l + ROW, .. and the groups l, l + ROW, .. of four
// consecutive quantised planes (one 8-byte index load per group, one 8-byte palette load per plane, all three channels in
// it).  A lane sums its retained planes, then its quantised planes, both ascending; row_sum adds the lanes: the order
// depends on (ROW, K, r) only.  AUX: the float kernel's three extra outputs, the same way (they depend on sigma and the
// geometry only, and sigma is the float tree's).
template <int ROW, bool AUX = false>
__global__ __launch_bounds__(kRenderThreads) void octree_render_quant_kernel(MaybeAux<QuantRenderArgs, AUX> A,
                                                                              float* __restrict__ out_rgb) {
  using G = RowGeom<ROW>;
  constexpr int kRow = ROW, kRaysPerBlock = G::kRaysPerBlock;
  constexpr int kQM = (7 + ROW - 1) / ROW;         // index groups per lane: Kq <= 25 -> at most 7 groups of four
  constexpr int kRM = (24 + ROW - 1) / ROW;        // retained planes per lane: r <= 24
  __shared__ int s_stack[kRaysPerBlock][kMaxD + 2];
  __shared__ float s_basis[kRaysPerBlock][25];
  const int row = threadIdx.x / kRow, l = threadIdx.x % kRow;
  float origin[3], dir[3], vdir[3];
  const RowId id = row_ray<ROW>(A, row, origin, dir, vdir);
  if (!id.active) return;                      // whole rows leave together; no block-level barrier below
  const int64_t ray = id.ray;

  const int K = A.tree.basis_dim, R = A.tree.n_retained, Kq = K - R, bits = A.tree.bits;
  const int groups = A.tree.idx_stride >> 2;
  const uint32_t id_mask = (1u << bits) - 1u;
  const float bg = A.opt.background_brightness;
  TreeRay r;
  to_tree_ray(origin, dir, A.tree.offset, A.tree.invradius, r);
  CellExit cell_exit;
  cell_exit.init(r.invdir);
  if (r.tmax < 0.0f || r.tmin > r.tmax) {
    for (int c = l; c < 3; c += kRow) out_rgb[ray * 3 + c] = bg;
    if constexpr (AUX)
      for (int c = l; c < 3; c += kRow) A.out[ray * 3 + c] = c == 2 ? INFINITY : 0.0f;
    return;
  }

  if (l == 0) sh_basis_dyn(K, vdir[0], vdir[1], vdir[2], s_basis[row]);
  __builtin_amdgcn_wave_barrier();
  float yr[kRM], yq[4 * kQM];                  // basis values of the planes this lane owns (0 past the end)
#pragma unroll
  for (int m = 0; m < kRM; ++m) yr[m] = (l + kRow * m) < R ? s_basis[row][l + kRow * m] : 0.0f;
#pragma unroll
  for (int j = 0; j < 4 * kQM; ++j) {
    const int q = 4 * (l + kRow * (j >> 2)) + (j & 3);
    yq[j] = q < Kq ? s_basis[row][R + q] : 0.0f;
  }
  const int32_t* __restrict__ child = A.tree.child;
  const float* __restrict__ sigma = A.tree.sigma;
  const u16x4* __restrict__ idx = reinterpret_cast<const u16x4*>(A.tree.idx);
  const f16x4* __restrict__ palette = reinterpret_cast<const f16x4*>(A.tree.palette);
  const f16x4* __restrict__ retained = reinterpret_cast<const f16x4*>(A.tree.retained);

  Marcher mk;
  mk.init(s_stack[row]);
  float t = r.tmin, light = 1.0f;
  float out[3] = {0.f, 0.f, 0.f};
  float aux[3] = {0.f, 0.f, INFINITY};           // AUX: alpha, depth, surface
  bool stopped = false;
  // the float kernel's software pipeline: sigma requested, the next sample located, then the current one shaded
  auto locate = [&](float tt, int64_t& leaf_o, float& delta_o) {
    locate_leaf(r, cell_exit, mk, child, A.opt.step_size, tt, leaf_o, delta_o);
  };
  int64_t leaf = 0;
  float delta_t = 0.0f;
  bool more = t < r.tmax;
  if (more) locate(t, leaf, delta_t);
  while (more) {
    const float sg = sigma[leaf];
    const float tn = t + delta_t;
    more = tn > t && tn < r.tmax;              // !(tn > t): step below the resolution of t, stop rather than spin
    const int64_t leaf_cur = leaf;
    const float delta_cur = delta_t;
    const float t_cur = t;
    if (more) locate(tn, leaf, delta_t);
    t = tn;
    if (sg > A.opt.sigma_thresh) {
      const float dtw = delta_cur * r.delta_scale;
      const float att = expf(-dtw * sg);
      const float weight = light * (1.0f - att);
      float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int m = 0; m < kRM; ++m) {
        const int b = l + kRow * m;
        if (b < R) {
          const f16x4 c = retained[leaf_cur * R + b];
          p0 += (float)c[0] * yr[m];
          p1 += (float)c[1] * yr[m];
          p2 += (float)c[2] * yr[m];
        }
      }
      const u16x4* __restrict__ ids = idx + leaf_cur * groups;
#pragma unroll
      for (int m = 0; m < kQM; ++m) {
        const int g = l + kRow * m;
        if (g < groups) {
          const u16x4 id = ids[g];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int q = 4 * g + e;
            if (q < Kq) {                      // the row's padding has no palette
              const f16x4 c = palette[((int64_t)q << bits) + ((uint32_t)id[e] & id_mask)];
              p0 += (float)c[0] * yq[4 * m + e];
              p1 += (float)c[1] * yq[4 * m + e];
              p2 += (float)c[2] * yq[4 * m + e];
            }
          }
        }
      }
      p0 = row_sum<ROW>(p0);
      p1 = row_sum<ROW>(p1);
      p2 = row_sum<ROW>(p2);
      const float c0 = 1.0f / (1.0f + expf(-p0)), c1 = 1.0f / (1.0f + expf(-p1)), c2 = 1.0f / (1.0f + expf(-p2));
      out[0] += weight * c0;
      out[1] += weight * c1;
      out[2] += weight * c2;
      light = light * att;
      if constexpr (AUX) {
        const float s = (t_cur + 0.5f * delta_cur) * r.delta_scale;
        aux[0] += weight;
        aux[1] += weight * s;
        if (light <= A.surface_thresh && aux[2] == INFINITY) aux[2] = s;
      }
      if (light <= A.opt.stop_thresh) {
        const float scale = 1.0f / (1.0f - light);
        out[0] *= scale; out[1] *= scale; out[2] *= scale;
        if constexpr (AUX) { aux[0] *= scale; aux[1] *= scale; }
        stopped = true;
        break;
      }
    }
  }
  if (!stopped) {
    out[0] += light * bg; out[1] += light * bg; out[2] += light * bg;
  }
  for (int c = l; c < 3; c += kRow) out_rgb[ray * 3 + c] = c == 0 ? out[0] : (c == 1 ? out[1] : out[2]);
  if constexpr (AUX)
    for (int c = l; c < 3; c += kRow) A.out[ray * 3 + c] = c == 0 ? aux[0] : (c == 1 ? aux[1] : aux[2]);
}

// ------------------------------------------------------------------------------------------
// per-leaf compositing weights (svox N3Tree.accumulate_weights; pxo_octree_weight_accum_* in plenoctree_octree.h)
// The forward renderer's march without shading, as octree_count_kernel repeats it (both on locate_leaf) -- same ray set-up (NDC included), leaf
// lookup, step rule, sigma test, attenuation, early stop and `!(tn > t)` guard, hence the same sample sequence -- and for
// every shaded sample its `weight`, light * (1 - expf(-(delta * delta_scale) * sigma)), merged into weights[leaf].  One thread
// per ray; in camera mode ray = (camera * H + py) * W + px over all cameras of c2w_all ([n_cams,12]).
//   OP 0  max: weights are >= 0, so their float order is the order of their bit patterns as signed integers (the weight-mask
//         marchers' atomicMax); a plain load in front keeps samples that cannot raise the value from issuing an atomic
//   OP 1  sum: float atomic add
// ------------------------------------------------------------------------------------------
struct WeightArgs {
  PxoTree tree;
  const float* c2w_all;                        // camera mode (non-NULL): [n_cams,12]
  float fx, fy;
  int W, H;
  const float* origins;                        // explicit rays: [n_rays,3] each
  const float* dirs;
  int64_t n_rays;                              // camera mode: n_cams * W * H
  PxoRenderOpts opt;
  PxoNdc ndc;                                  // width == 0: world-space rays
  float* weights;                              // [n_internal*8]
};

template <int OP>
__global__ __launch_bounds__(256) void octree_weight_kernel(WeightArgs A) {
  __shared__ int s_stack[256][kMaxD + 2];
  const int64_t ray = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (ray >= A.n_rays) return;                 // no barrier below
  float origin[3], dir[3];
  if (A.c2w_all) {
    const int64_t per_cam = (int64_t)A.W * A.H;
    const int64_t cam = ray / per_cam;
    const int pix = (int)(ray - cam * per_cam);
    camera_ray(A.c2w_all + cam * 12, A.fx, A.fy, A.W, A.H, pix % A.W, pix / A.W, origin, dir);
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      origin[a] = A.origins[ray * 3 + a];
      dir[a] = A.dirs[ray * 3 + a];
    }
  }
  bool ndc_miss = false;
  if (A.ndc.width > 0) ndc_miss = !ndc_ray(A.ndc, origin, dir);
  TreeRay r;
  to_tree_ray(origin, dir, A.tree.offset, A.tree.invradius, r);
  CellExit cell_exit;
  cell_exit.init(r.invdir);
  if (ndc_miss || r.tmax < 0.0f || r.tmin > r.tmax) return;
  const int D = A.tree.data_dim;
  const float* __restrict__ data = A.tree.data;
  const int32_t* __restrict__ child = A.tree.child;
  float* weights = A.weights;
  Marcher mk;
  mk.init(s_stack[threadIdx.x]);
  float t = r.tmin, light = 1.0f;
  while (t < r.tmax) {
    int64_t leaf;
    float delta_t;
    locate_leaf(r, cell_exit, mk, child, A.opt.step_size, t, leaf, delta_t);
    const float sg = data[leaf * D + D - 1];
    if (sg > A.opt.sigma_thresh) {
      const float dtw = delta_t * r.delta_scale;
      const float att = expf(-dtw * sg);
      const float weight = light * (1.0f - att);
      if (OP == 0) {
        if (weight > weights[leaf]) atomicMax(reinterpret_cast<int*>(weights + leaf), __float_as_int(weight));
      } else {
        if (weight > 0.0f) unsafeAtomicAdd(weights + leaf, weight);
      }
      light = light * att;
      if (light <= A.opt.stop_thresh) break;
    }
    const float tn = t + delta_t;
    if (!(tn > t)) break;
    t = tn;
  }
}

// ------------------------------------------------------------------------------------------
// structural collapse (pxo_tree_collapse_mark / _emit in plenoctree_octree.h)
// ------------------------------------------------------------------------------------------
// one pass per depth, deepest first: a node of depth d is dead when each of its cells is a leaf with keep == 0 or points
// to a (depth d + 1, already decided) dead node.  Nodes are picked by their stored depth, not by their position.
__global__ void tree_collapse_mark_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ parent_depth,
                                          const uint8_t* __restrict__ keep, int64_t n, int d, uint8_t* __restrict__ node_dead) {
  const int64_t node = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (node >= n || parent_depth[node * 2 + 1] != d) return;
  bool dead = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int skip = child[node * 8 + c];
    dead = dead && (skip == 0 ? keep[node * 8 + c] == 0 : node_dead[node + skip] != 0);
  }
  node_dead[node] = dead ? 1 : 0;
}

// a cell of a surviving node keeps its row unless it is a dead leaf or pointed to a dead node
__device__ __forceinline__ bool collapse_cell_live(const int32_t* __restrict__ child, const uint8_t* __restrict__ keep,
                                                   const uint8_t* __restrict__ node_dead, int64_t cell) {
  const int skip = child[cell];
  return skip == 0 ? keep[cell] != 0 : node_dead[(cell >> 3) + skip] == 0;
}

// one thread per old cell: child offsets between the survivors' new positions; cell 0 also writes the node's own records
__global__ void tree_collapse_struct_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ parent_depth,
                                            const uint8_t* __restrict__ node_dead, const int64_t* __restrict__ new_index,
                                            int64_t n, int32_t* __restrict__ new_child, int32_t* __restrict__ new_parent_depth,
                                            int64_t* __restrict__ old2new) {
  const int64_t cell = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (cell >= n * 8) return;
  const int64_t node = cell >> 3;
  const int c = (int)(cell & 7);
  const bool dead = node_dead[node] != 0;
  if (c == 0) old2new[node] = dead ? -1 : new_index[node];
  if (dead) return;
  const int64_t m = new_index[node];
  const int skip = child[cell];
  new_child[m * 8 + c] = (skip != 0 && node_dead[node + skip] == 0) ? (int32_t)(new_index[node + skip] - m) : 0;
  if (c == 0) {
    const int32_t p = parent_depth[node * 2];            // the parent of a survivor survives; the root's record is (0, 0)
    new_parent_depth[m * 2] = (int32_t)(new_index[p >> 3] * 8 + (p & 7));
    new_parent_depth[m * 2 + 1] = parent_depth[node * 2 + 1];
  }
}

// one thread per old data element: survivors' rows move to their new place, rows of dead leaf cells become zero
__global__ void tree_collapse_data_kernel(const int32_t* __restrict__ child, const float* __restrict__ data, int D,
                                          const uint8_t* __restrict__ keep, const uint8_t* __restrict__ node_dead,
                                          const int64_t* __restrict__ new_index, int64_t n, float* __restrict__ new_data) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * 8 * D) return;
  const int64_t cell = i / D;
  const int64_t node = cell >> 3;
  if (node_dead[node]) return;
  const float v = collapse_cell_live(child, keep, node_dead, cell) ? data[i] : 0.0f;
  new_data[(new_index[node] * 8 + (cell & 7)) * D + (i - cell * D)] = v;
}

// ------------------------------------------------------------------------------------------
// scene: several trees under similarity transforms, marched together (plenoctree_octree.h, "scene")
// ------------------------------------------------------------------------------------------
// One ray per row of 4 lanes, 64 rays per workgroup, as the forward renderer at its default; row_ray deals the rays.  The four
// lanes of a row run the same march (row-uniform control flow) and split a leaf's coefficients exactly as
// octree_render_kernel<0, 4, true, K> does, with K a run-time value: the same products in the same order, so a one-instance
// identity scene returns that kernel's bits.
// Eight instances' ray constants and march state do not fit in registers beside an SH25 dot, and a loop over instances cannot
// index registers: all per-instance state of a ray lives in dynamic LDS, sized by the launch's instance count.  Per instance:
//   stack  int   [64 rays][kMaxD + 2]   the Marcher's node path (ray stride 12 words: 16 rays of a wave on 16 distinct banks)
//   basis  float [64 rays][25]          SH basis on the rotated view direction (stride 25: odd)
//   field  word  [kSceneFields][64 rays] ray constants, march state and the round's offers, field-major (a wave's 16 rays read
//                                        16 consecutive words; the 4 lanes of a row the same word: a broadcast)
// = 4 * (12 + 25 + kSceneFields) = 236 bytes per ray and instance, 15104 per workgroup and instance (8 instances: 120832).
// Every lane of a row writes the same values to the row's words, so no lane waits for another except for the basis (lane
// i % 4 evaluates instance i's), which a wave barrier orders.
constexpr int kSceneRow = 4;
constexpr int kSceneRays = kRenderThreads / kSceneRow;
enum SceneField {
  kScO = 0, kScD = 3, kScInv = 6,               // tree-space origin, unit direction, 1 / (d + 1e-9)
  kScTmax = 9, kScC, kScEnter, kScT,           // tmax, c = scale * delta_scale, enter = tmin * c, tt (tmin until entered)
  kScPX, kScPY, kScPZ, kScDepth,               // Marcher: the previous sample's quantised position and depth (-1: no sample yet)
  kScState,                                    // 0 done, 1 waiting, 2 inside, 3 inside and live in this round
  kScLeaf, kScDelta, kScStep,                  // this round: leaf, tree-space step, the offer (step or gap) in world length
  kScTau,                                      // this round: tau_i of a live instance
  kSceneFields
};
constexpr int kSceneWordsPerRay = kMaxD + 2 + 25 + kSceneFields;
static_assert(kSceneFields == 22 && kSceneWordsPerRay == 59, "scene LDS layout (plenoctree_octree.h, DESIGN)");

struct SceneArgs {
  const PxoInstance* inst;                     // device array [n]
  int n;
  PxoCamera cam;
  int has_cam;
  const float* origins;
  const float* dirs;
  const float* viewdirs;
  int64_t B;
  PxoRenderOpts opt;
};

__global__ __launch_bounds__(kRenderThreads) void scene_render_kernel(SceneArgs A, float* __restrict__ out_rgb) {
  extern __shared__ __attribute__((aligned(16))) int s_scene[];
  const int n = A.n;
  const int row = threadIdx.x / kSceneRow, l = threadIdx.x % kSceneRow;
  int* const s_stack = s_scene + row * (kMaxD + 2);                                  // + i * kSceneRays * (kMaxD + 2)
  float* const s_basis = reinterpret_cast<float*>(s_scene + n * kSceneRays * (kMaxD + 2)) + row * 25;   // + i * kSceneRays * 25
  int* const s_field = s_scene + n * kSceneRays * (kMaxD + 2 + 25) + row;            // + (i * kSceneFields + f) * kSceneRays
  auto fi = [&](int i, int f) -> int& { return s_field[(i * kSceneFields + f) * kSceneRays]; };
  auto ff = [&](int i, int f) -> float& { return reinterpret_cast<float*>(s_field)[(i * kSceneFields + f) * kSceneRays]; };

  float origin[3], dir[3], vdir[3];
  const RowId id = row_ray<kSceneRow>(A, row, origin, dir, vdir);
  if (!id.active) return;                      // whole rows leave together; only wave barriers below
  const int64_t ray = id.ray;
  const float bg = A.opt.background_brightness;

  // ---- set-up: the ray in every instance's frame ----
  float w = INFINITY;
  for (int i = 0; i < n; ++i) {
    const PxoInstance& I = A.inst[i];
    float q[3], oi[3], di[3], vi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = origin[a] - I.trans[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float* m = I.rot_t + 3 * a;
      oi[a] = ((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]) * I.inv_scale;
      di[a] = (m[0] * dir[0] + m[1] * dir[1]) + m[2] * dir[2];
      vi[a] = (m[0] * vdir[0] + m[1] * vdir[1]) + m[2] * vdir[2];
    }
    TreeRay r;
    to_tree_ray(oi, di, I.tree.offset, I.tree.invradius, r);
    const bool hit = !(r.tmax < 0.0f || r.tmin > r.tmax) && r.tmin < r.tmax;
    const float c = I.scale * r.delta_scale;
    const float enter = r.tmin * c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ff(i, kScO + a) = r.o[a];
      ff(i, kScD + a) = r.d[a];
      ff(i, kScInv + a) = r.invdir[a];
    }
    ff(i, kScTmax) = r.tmax;
    ff(i, kScC) = c;
    ff(i, kScEnter) = enter;
    ff(i, kScT) = r.tmin;
    fi(i, kScPX) = 0; fi(i, kScPY) = 0; fi(i, kScPZ) = 0;
    fi(i, kScDepth) = -1;
    fi(i, kScState) = hit ? 1 : 0;
    s_stack[i * kSceneRays * (kMaxD + 2)] = 0;
    if (hit) w = fminf(w, enter);
    if (hit && l == (i & (kSceneRow - 1))) sh_basis_dyn(I.tree.basis_dim, vi[0], vi[1], vi[2], s_basis + i * kSceneRays * 25);
  }
  __builtin_amdgcn_wave_barrier();
  if (!(w < INFINITY)) {                       // no instance is hit
    for (int c = l; c < 3; c += kSceneRow) out_rgb[ray * 3 + c] = bg;
    return;
  }

  float light = 1.0f;
  float out[3] = {0.f, 0.f, 0.f};
  bool stopped = false;
  while (true) {
    // ---- offers: a located step from every inside instance, the gap from every waiting one ----
    float d_min = INFINITY, next_enter = INFINITY;
    bool any_inside = false;
    for (int i = 0; i < n; ++i) {
      int st = fi(i, kScState);
      if (st == 0) continue;
      const float enter = ff(i, kScEnter);
      if (st == 1 && enter <= w) st = 2;
      if (st >= 2) {
        TreeRay r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          r.o[a] = ff(i, kScO + a);
          r.d[a] = ff(i, kScD + a);
          r.invdir[a] = ff(i, kScInv + a);
        }
        CellExit cell_exit;
        cell_exit.init(r.invdir);
        Marcher mk;
        mk.stack = s_stack + i * kSceneRays * (kMaxD + 2);
        mk.last_depth = fi(i, kScDepth);
        mk.first = mk.last_depth < 0;
        mk.pX = (uint32_t)fi(i, kScPX); mk.pY = (uint32_t)fi(i, kScPY); mk.pZ = (uint32_t)fi(i, kScPZ);
        int64_t leaf;
        float delta;
        locate_leaf(r, cell_exit, mk, A.inst[i].tree.child, A.opt.step_size, ff(i, kScT), leaf, delta);
        fi(i, kScPX) = (int)mk.pX; fi(i, kScPY) = (int)mk.pY; fi(i, kScPZ) = (int)mk.pZ;
        fi(i, kScDepth) = mk.last_depth;
        const float step = delta * ff(i, kScC);
        fi(i, kScLeaf) = (int)leaf;             // n_internal < 2^28: node * 8 + cell fits
        ff(i, kScDelta) = delta;
        ff(i, kScStep) = step;
        fi(i, kScState) = 2;
        d_min = fminf(d_min, step);
        any_inside = true;
      } else {
        const float gap = enter - w;
        ff(i, kScStep) = gap;
        d_min = fminf(d_min, gap);
        next_enter = fminf(next_enter, enter);
      }
    }
    if (!any_inside) {
      if (!(next_enter < INFINITY)) break;      // nothing waiting either
      w = next_enter;
      continue;
    }

    // ---- one sample ----
    float tau = 0.0f;
    bool any_live = false;
    for (int i = 0; i < n; ++i) {
      if (fi(i, kScState) != 2) continue;
      const PxoInstance& I = A.inst[i];
      const float sg = I.tree.data[(int64_t)fi(i, kScLeaf) * I.tree.data_dim + I.tree.data_dim - 1];
      if (sg > A.opt.sigma_thresh) {
        const float tau_i = (d_min * I.inv_scale) * sg;
        ff(i, kScTau) = tau_i;
        fi(i, kScState) = 3;
        tau = tau + tau_i;
        any_live = true;
      }
    }
    if (any_live && tau > 0.0f) {
      const float att = expf(-tau);
      const float weight = light * (1.0f - att);
      for (int i = 0; i < n; ++i) {
        if (fi(i, kScState) != 3) continue;
        const PxoInstance& I = A.inst[i];
        const int K = I.tree.basis_dim;
        const float* __restrict__ val = I.tree.data + (int64_t)fi(i, kScLeaf) * I.tree.data_dim;
        const float* Y = s_basis + i * kSceneRays * 25;
        const int chG = K >> 2, chR = K & 3;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int m = 0; m < 2; ++m) {           // K <= 25: at most 6 whole groups of four, 2 per lane
          const int g = l + kSceneRow * m;
          if (g < chG) {
            const f32x4u c0 = *reinterpret_cast<const f32x4u*>(val + 4 * g);
            const f32x4u c1 = *reinterpret_cast<const f32x4u*>(val + K + 4 * g);
            const f32x4u c2 = *reinterpret_cast<const f32x4u*>(val + 2 * K + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float b = Y[4 * g + e];
              p0 += c0[e] * b;
              p1 += c1[e] * b;
              p2 += c2[e] * b;
            }
          }
        }
        if (l < chR) {
          const int k = 4 * chG + l;
          const float b = Y[k];
          p0 += val[k] * b;
          p1 += val[K + k] * b;
          p2 += val[2 * K + k] * b;
        }
        p0 = row_sum<kSceneRow>(p0);
        p1 = row_sum<kSceneRow>(p1);
        p2 = row_sum<kSceneRow>(p2);
        const float c0 = 1.0f / (1.0f + expf(-p0)), c1 = 1.0f / (1.0f + expf(-p1)), c2 = 1.0f / (1.0f + expf(-p2));
        const float share = weight * (ff(i, kScTau) / tau);
        out[0] += share * c0;
        out[1] += share * c1;
        out[2] += share * c2;
      }
      light = light * att;
      if (light <= A.opt.stop_thresh) {
        const float scale = 1.0f / (1.0f - light);
        out[0] *= scale; out[1] *= scale; out[2] *= scale;
        stopped = true;
        break;
      }
    }

    // ---- advance ----
    float snap = -INFINITY;
    for (int i = 0; i < n; ++i) {
      const int st = fi(i, kScState);
      if (st >= 2) {
        const float tt = ff(i, kScT);
        const float tn = ff(i, kScStep) == d_min ? tt + ff(i, kScDelta) : tt + d_min / ff(i, kScC);
        if (!(tn > tt) || tn >= ff(i, kScTmax)) {
          fi(i, kScState) = 0;
        } else {
          ff(i, kScT) = tn;
          fi(i, kScState) = 2;
        }
      } else if (st == 1 && ff(i, kScStep) == d_min) {
        snap = fmaxf(snap, ff(i, kScEnter));
      }
    }
    w = snap > -INFINITY ? snap : w + d_min;
  }
  if (!stopped) {
    out[0] += light * bg; out[1] += light * bg; out[2] += light * bg;
  }
  for (int c = l; c < 3; c += kSceneRow) out_rgb[ray * 3 + c] = c == 0 ? out[0] : (c == 1 ? out[1] : out[2]);
}

}  // namespace pxo

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace pxo;

static inline int64_t blocks_for(int64_t n, int threads) { return (n + threads - 1) / threads; }

// ---- renderer launches (templates: outside the C linkage block) ----
// What the renderers of every form share of a launch at `row` lanes per ray: the checks on the camera or the ray arrays,
// the rays' part of the argument block (Args: a FwdBlock or QuantRenderArgs) and the block count.
template <typename Args>
static int launch_shape(const PxoCamera* cam, const float* origins, const float* dirs, const float* viewdirs, int64_t B, int row,
                        const char* who, Args& A, unsigned& grid) {
  PXO_REQUIRE(B >= 0, "%s: B < 0", who);
  A.B = B;
  A.has_cam = cam != nullptr;
  int64_t blocks;
  if (cam) {
    PXO_REQUIRE(cam->c2w && cam->width >= 1 && cam->height >= 1 && cam->fx > 0.0f && cam->fy > 0.0f, "%s: bad camera", who);
    PXO_REQUIRE(B == (int64_t)cam->width * cam->height, "%s: B must be width*height in camera mode", who);
    A.cam = *cam;
    A.origins = A.dirs = A.viewdirs = nullptr;
    const int tx = 2 * patch_wtx(row), ty = 2 * (64 / row / patch_wtx(row));      // a block's 2 x 2 patches (row_ray)
    blocks = (int64_t)((cam->width + tx - 1) / tx) * ((cam->height + ty - 1) / ty);
  } else {
    PXO_REQUIRE(B == 0 || (origins && dirs && viewdirs), "%s: null ray arrays", who);
    A.cam = PxoCamera{};
    A.origins = origins; A.dirs = dirs; A.viewdirs = viewdirs;
    blocks = blocks_for(B, kRenderThreads / row);
  }
  PXO_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many rays for one launch", who);
  grid = (unsigned)blocks;
  return PXO_OK;
}

// The forward launch of one argument block at `row` lanes per ray.  Rows of float or float16, 4 lanes: the channel-aligned
// kernel with the tree's basis_dim as a compile-time constant (check_format has admitted these five values only, so there
// is no run-time-K variant); 8 / 16 lanes: groups of four consecutive floats.  The palette form has one kernel per `row`.
template <typename Block, bool AUX, bool FOOT = false>
static void launch_fwd(const MaybeFoot<MaybeAux<Block, AUX>, FOOT>& A, int row, unsigned grid, float* out_rgb, void* stream) {
  static_assert(!FOOT || std::is_same<Block, RenderArgs>::value, "footprint depth: the float tree only");
  if constexpr (std::is_same<Block, QuantRenderArgs>::value) {
    const auto kernel = row == 4   ? octree_render_quant_kernel<4, AUX>
                        : row == 8 ? octree_render_quant_kernel<8, AUX>
                                   : octree_render_quant_kernel<16, AUX>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRenderThreads), 0, (hipStream_t)stream, A, out_rgb);
  } else {
    using ST = std::conditional_t<std::is_same<Block, RenderArgs>::value, float, _Float16>;
    auto kernel = row == 8 ? octree_render_kernel<0, 8, true, 0, AUX, ST, FOOT> : octree_render_kernel<0, 16, true, 0, AUX, ST, FOOT>;
    if (row == 4) {
      switch (A.tree.basis_dim) {
        case 1: kernel = octree_render_kernel<0, 4, true, 1, AUX, ST, FOOT>; break;
        case 4: kernel = octree_render_kernel<0, 4, true, 4, AUX, ST, FOOT>; break;
        case 9: kernel = octree_render_kernel<0, 4, true, 9, AUX, ST, FOOT>; break;
        case 16: kernel = octree_render_kernel<0, 4, true, 16, AUX, ST, FOOT>; break;
        default: kernel = octree_render_kernel<0, 4, true, 25, AUX, ST, FOOT>; break;
      }
    }
    const float* none = nullptr;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRenderThreads), 0, (hipStream_t)stream, A, out_rgb, none, none, (float*)nullptr);
  }
}

// The 4-lane backward kernel for `wc_rows` rows of write-combining cache (0: direct scatter) and the cache's update form.
using Bwd4Kernel = void (*)(RenderArgs, const float*, const float*, float*);
template <int KF>
static Bwd4Kernel bwd4_kernel(int wc_rows, bool ray_parallel) {
  switch (wc_rows) {
    case 4: return ray_parallel ? octree_render_bwd4_kernel<KF, 4, 1> : octree_render_bwd4_kernel<KF, 4, 0>;
    case 8: return ray_parallel ? octree_render_bwd4_kernel<KF, 8, 1> : octree_render_bwd4_kernel<KF, 8, 0>;
    case 16: return ray_parallel ? octree_render_bwd4_kernel<KF, 16, 1> : octree_render_bwd4_kernel<KF, 16, 0>;
    case 32: return ray_parallel ? octree_render_bwd4_kernel<KF, 32, 1> : octree_render_bwd4_kernel<KF, 32, 0>;
    case 64: return ray_parallel ? octree_render_bwd4_kernel<KF, 64, 1> : octree_render_bwd4_kernel<KF, 64, 0>;
    default: return octree_render_bwd4_kernel<KF, 0, 0>;
  }
}

extern "C" {

int pxo_threshold_mask(const float* value, int64_t n, float thresh, uint8_t* mask, void* stream) {
  PXO_REQUIRE(n >= 0, "pxo_threshold_mask: n < 0");
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(value && mask, "pxo_threshold_mask: null pointer");
  hipLaunchKernelGGL(threshold_mask_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, value, n,
                     thresh, mask);
  return check_launch("threshold_mask");
}

int pxo_tree_workspace_bytes(int depth, size_t* bytes) {
  PXO_REQUIRE(depth >= 1 && depth <= kMaxD, "pxo_tree_workspace_bytes: depth %d outside [1,%d]", depth, kMaxD);
  PXO_REQUIRE(bytes, "pxo_tree_workspace_bytes: null pointer");
  *bytes = (size_t)tree_ws(depth).total;
  return PXO_OK;
}

static int scan_level(const uint8_t* occ, int64_t n, uint32_t* bsum, int32_t* rank, int64_t* count, hipStream_t s) {
  const int64_t nb = blocks_for(n, kScanElems);
  hipLaunchKernelGGL(scan_blocksum_kernel, dim3((unsigned)nb), dim3(256), 0, s, occ, n, bsum);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, s, bsum, nb, count);
  hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)nb), dim3(256), 0, s, occ, n, (const uint32_t*)bsum, rank);
  return check_launch("tree scan");
}

int pxo_tree_count_nodes(const uint8_t* mask, int depth, void* ws, size_t ws_bytes, int64_t* level_nodes, void* stream) {
  PXO_REQUIRE(depth >= 1 && depth <= kMaxD, "pxo_tree_count_nodes: depth %d outside [1,%d]", depth, kMaxD);
  PXO_REQUIRE(mask && ws && level_nodes, "pxo_tree_count_nodes: null pointer");
  const TreeWs w = tree_ws(depth);
  if (ws_bytes < (size_t)w.total) {
    set_error("pxo_tree_count_nodes: workspace %zu < %lld", ws_bytes, (long long)w.total);
    return PXO_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  uint8_t* occ_d = (uint8_t*)(base + w.occ_off[depth]);
  hipLaunchKernelGGL(pyramid_base_kernel, dim3((unsigned)blocks_for(pow8(depth), 256)), dim3(256), 0, s, mask, depth, occ_d);
  for (int d = depth - 1; d >= 1; --d) {
    hipLaunchKernelGGL(pyramid_up_kernel, dim3((unsigned)blocks_for(pow8(d), 256)), dim3(256), 0, s,
                       (const uint8_t*)(base + w.occ_off[d + 1]), pow8(d), (uint8_t*)(base + w.occ_off[d]));
  }
  int64_t* counts = (int64_t*)(base + w.count_off);
  for (int d = 1; d <= depth; ++d) {
    const int rc = scan_level((const uint8_t*)(base + w.occ_off[d]), pow8(d), (uint32_t*)(base + w.bsum_off),
                              (int32_t*)(base + w.rank_off[d]), counts + d, s);
    if (rc) return rc;
  }
  if (hipMemcpyAsync(level_nodes + 1, counts + 1, sizeof(int64_t) * depth, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("pxo_tree_count_nodes: %s", hipGetErrorString(hipGetLastError()));
    return PXO_ERR_HIP;
  }
  level_nodes[0] = 1;
  return PXO_OK;
}

int pxo_tree_build(const void* ws, size_t ws_bytes, int depth, const int64_t* level_nodes, int32_t* child,
                   int32_t* parent_depth, void* stream) {
  PXO_REQUIRE(depth >= 1 && depth <= kMaxD, "pxo_tree_build: depth %d outside [1,%d]", depth, kMaxD);
  PXO_REQUIRE(ws && level_nodes && child && parent_depth, "pxo_tree_build: null pointer");
  const TreeWs w = tree_ws(depth);
  if (ws_bytes < (size_t)w.total) {
    set_error("pxo_tree_build: workspace %zu < %lld", ws_bytes, (long long)w.total);
    return PXO_ERR_WORKSPACE;
  }
  LevelPtrs lv{};
  const char* base = (const char*)ws;
  int64_t start = 0;
  for (int d = 0; d <= depth; ++d) {
    lv.start[d] = start;
    start += level_nodes[d];
    if (d >= 1) {
      lv.occ[d] = (const uint8_t*)(base + w.occ_off[d]);
      lv.rank[d] = (const int32_t*)(base + w.rank_off[d]);
    }
  }
  PXO_REQUIRE(start < ((int64_t)1 << 28), "pxo_tree_build: %lld nodes exceed the int32 packed-index range", (long long)start);
  for (int d = 0; d <= depth; ++d) {
    if (level_nodes[d] == 0) break;
    hipLaunchKernelGGL(tree_emit_kernel, dim3((unsigned)blocks_for(pow8(d), 256)), dim3(256), 0, (hipStream_t)stream, lv, d,
                       depth, child, parent_depth);
  }
  return check_launch("tree_emit");
}

int pxo_tree_sample_cells(const int32_t* parent_depth, int64_t node0, int64_t n_nodes, int S, const float* u,
                          const float offset[3], const float invradius[3], float* points, void* stream) {
  PXO_REQUIRE(n_nodes >= 0 && node0 >= 0 && S >= 1, "pxo_tree_sample_cells: bad sizes");
  if (n_nodes == 0) return PXO_OK;
  PXO_REQUIRE(parent_depth && u && offset && invradius && points, "pxo_tree_sample_cells: null pointer");
  const int64_t n = n_nodes * 8 * S;
  hipLaunchKernelGGL(tree_sample_cells_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     parent_depth, node0, n_nodes, S, u, offset[0], offset[1], offset[2], invradius[0], invradius[1],
                     invradius[2], points);
  return check_launch("tree_sample_cells");
}

int pxo_tree_sample_leaves(const int32_t* parent_depth, const int64_t* packed, int64_t n_cells, int S, const float* u,
                           const float offset[3], const float invradius[3], float* points, void* stream) {
  PXO_REQUIRE(n_cells >= 0 && S >= 1, "pxo_tree_sample_leaves: bad sizes");
  if (n_cells == 0) return PXO_OK;
  PXO_REQUIRE(parent_depth && packed && u && offset && invradius && points, "pxo_tree_sample_leaves: null pointer");
  const int64_t n = n_cells * S;
  hipLaunchKernelGGL(tree_sample_leaves_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     parent_depth, packed, n_cells, S, u, offset[0], offset[1], offset[2], invradius[0], invradius[1],
                     invradius[2], points);
  return check_launch("tree_sample_leaves");
}

int pxo_tree_query(const int32_t* child, const float* points, int64_t n, const float offset[3], const float invradius[3],
                   int64_t* packed, void* stream) {
  PXO_REQUIRE(n >= 0, "pxo_tree_query: n < 0");
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(child && points && offset && invradius && packed, "pxo_tree_query: null pointer");
  hipLaunchKernelGGL(tree_query_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, child, points,
                     n, offset[0], offset[1], offset[2], invradius[0], invradius[1], invradius[2], packed);
  return check_launch("tree_query");
}

int pxo_tree_relu_sigma(float* data, int64_t n_cells, int data_dim, void* stream) {
  PXO_REQUIRE(n_cells >= 0 && data_dim >= 1, "pxo_tree_relu_sigma: bad sizes");
  if (n_cells == 0) return PXO_OK;
  PXO_REQUIRE(data, "pxo_tree_relu_sigma: null pointer");
  hipLaunchKernelGGL(tree_relu_sigma_kernel, dim3((unsigned)blocks_for(n_cells, 256)), dim3(256), 0, (hipStream_t)stream, data,
                     n_cells, data_dim);
  return check_launch("tree_relu_sigma");
}

static int check_opts(const PxoRenderOpts* o, const char* who) {
  PXO_REQUIRE(o, "%s: null options", who);
  PXO_REQUIRE(o->step_size > 0.0f, "%s: step_size must be > 0 (marching would not advance)", who);
  return PXO_OK;
}

int pxo_grid_weight_workspace_bytes(int reso, size_t* bytes) {
  PXO_REQUIRE(reso >= 1 && reso <= 2048 && bytes, "pxo_grid_weight_workspace_bytes: bad arguments");
  *bytes = (reso % 4 == 0) ? (size_t)2 * reso * reso * reso * sizeof(float) + 256 : 0;   // bricked sigma, bricked weights, a counter
  return PXO_OK;
}

static int g_gw_marcher = -1;   // -1: chosen on the device; 0 / 1: forced (pxo_octree_set_tuning)
static int g_gw_tile_order = 0; // gw_tile: 0 linear, 1 XCD supertiles (PXO_TUNE_GW_TILE_ORDER)

static const PxoNdc kNoNdc = {0, 0, 0.0f, 0.0f};   // PxoNdc::width == 0: a world-space launch

static int check_ndc(const PxoNdc* ndc, const char* who) {
  PXO_REQUIRE(ndc, "%s: null ndc", who);
  PXO_REQUIRE(ndc->width >= 1 && ndc->height >= 1, "%s: ndc width %d / height %d must be >= 1", who, ndc->width, ndc->height);
  PXO_REQUIRE(ndc->focal > 0.0f && ndc->near > 0.0f, "%s: ndc focal %g and near %g must be > 0", who, (double)ndc->focal,
              (double)ndc->near);
  return PXO_OK;
}

static int grid_weight_render_impl(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                                   int width, int height, const PxoRenderOpts* opts, const float offset[3],
                                   const float invradius[3], float* grid_weight, void* ws, size_t ws_bytes, void* stream,
                                   const PxoNdc& ndc) {
  if (int rc = check_opts(opts, "pxo_grid_weight_render")) return rc;
  PXO_REQUIRE(reso >= 1 && reso <= 2048 && n_cams >= 0 && width >= 1 && height >= 1, "pxo_grid_weight_render: bad sizes");
  PXO_REQUIRE(fx > 0.0f && fy > 0.0f, "pxo_grid_weight_render: focal length must be > 0");
  if (n_cams == 0) return PXO_OK;
  PXO_REQUIRE(sigma_grid && c2w_all && offset && invradius && grid_weight, "pxo_grid_weight_render: null pointer");
  Vec3 o{{offset[0], offset[1], offset[2]}}, ir{{invradius[0], invradius[1], invradius[2]}};
  const int64_t tiles = (int64_t)((width + 15) / 16) * ((height + 15) / 16);
  PXO_REQUIRE(tiles * n_cams < ((int64_t)1 << 31), "pxo_grid_weight_render: too many tiles for one launch");
  const unsigned gw_grid = (unsigned)(tiles * n_cams);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)reso * reso * reso;
  if (reso % 4 != 0) {   // grids that do not tile into bricks (never the case for 2^(depth+1), depth >= 1)
    hipLaunchKernelGGL((grid_weight_kernel<false, false>), dim3(gw_grid), dim3(256), 0, s, sigma_grid, reso, c2w_all,
                       n_cams, fx, fy, width, height, *opts, o, ir, reinterpret_cast<int*>(grid_weight), ndc);
    return check_launch("grid_weight_render");
  }
  const size_t need = (size_t)2 * n * sizeof(float) + 256;
  if (!ws || ws_bytes < need) {
    set_error("pxo_grid_weight_render: workspace %zu < %zu", ws_bytes, need);
    return PXO_ERR_WORKSPACE;
  }
  float* sigma_b = reinterpret_cast<float*>(ws);
  float* weight_b = sigma_b + n;
  unsigned long long* occupied = reinterpret_cast<unsigned long long*>(weight_b + n);
  if (hipMemsetAsync(weight_b, 0, (size_t)n * sizeof(float) + 256, s) != hipSuccess) {
    set_error("pxo_grid_weight_render: hipMemsetAsync failed");
    return PXO_ERR_HIP;
  }
  const int64_t brick_blocks = blocks_for(n, 256);
  hipLaunchKernelGGL(brick_sigma_kernel, dim3((unsigned)(brick_blocks < 8192 ? brick_blocks : 8192)), dim3(256), 0, s, sigma_grid,
                     reso, sigma_b, opts->sigma_thresh, occupied);
  const bool pow2 = (reso & (reso - 1)) == 0 && reso <= 1024;
  // pxo_octree_set_tuning(PXO_TUNE_GW_MARCHER, 1 | 0) forces the slab-staged / the per-sample marcher (A/B runs, the
  // equality test); default -1: chosen on the device by the fraction of voxels above sigma_thresh (GwSelect).  Slab window width measured at 4 / 5 / 6 bricks:
  // 1.245 / 1.257 / 1.262 ms per camera (the staging is not what bounds the marcher); 6 keeps nearly every sample of a tile inside.
  const int force = g_gw_marcher;
  if (pow2) {
    const int64_t per_cam = gw_blocks_per_cam((width + 15) / 16, (height + 15) / 16, g_gw_tile_order);
    PXO_REQUIRE(per_cam * n_cams < ((int64_t)1 << 31), "pxo_grid_weight_render: too many tiles for one launch");
    hipLaunchKernelGGL(grid_weight_pow2_kernel, dim3((unsigned)(per_cam * n_cams)), dim3(256), 0, s, (const float*)sigma_b, reso, c2w_all, n_cams, fx,
                       fy, width, height, *opts, o, ir, reinterpret_cast<int*>(weight_b), GwSelect{occupied, n, force, g_gw_tile_order}, ndc);
  }
  else
    hipLaunchKernelGGL((grid_weight_kernel<true, false>), dim3(gw_grid), dim3(256), 0, s, (const float*)sigma_b, reso, c2w_all,
                       n_cams, fx, fy, width, height, *opts, o, ir, reinterpret_cast<int*>(weight_b), ndc);
  hipLaunchKernelGGL(unbrick_max_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, s, (const float*)weight_b, reso,
                     grid_weight);
  return check_launch("grid_weight_render");
}

int pxo_grid_weight_render(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                           int width, int height, const PxoRenderOpts* opts, const float offset[3],
                           const float invradius[3], float* grid_weight, void* ws, size_t ws_bytes, void* stream) {
  return grid_weight_render_impl(sigma_grid, reso, c2w_all, n_cams, fx, fy, width, height, opts, offset, invradius, grid_weight,
                                 ws, ws_bytes, stream, kNoNdc);
}

// the same launches -- either marcher, either tile order, bricked or not -- with the NDC set-up switched on
int pxo_grid_weight_render_ndc(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                               int width, int height, const PxoRenderOpts* opts, const float offset[3],
                               const float invradius[3], float* grid_weight, void* ws, size_t ws_bytes, void* stream,
                               const PxoNdc* ndc) {
  if (int rc = check_ndc(ndc, "pxo_grid_weight_render_ndc")) return rc;
  return grid_weight_render_impl(sigma_grid, reso, c2w_all, n_cams, fx, fy, width, height, opts, offset, invradius, grid_weight,
                                 ws, ws_bytes, stream, *ndc);
}

// Lanes per ray of the renderer launches.  Measured on the 512^3 / 800x800 / SH16 benchmark (profiles/README.md):
// forward 3.88 / 3.36 / 4.23 ms for 16 / 8 / 4 lanes (8 lanes: twice the rays in flight per wave, half the
// duplicated traversal arithmetic, coefficient rows still 32-byte coalesced); backward 10.9 / 14.0 / 22.1 ms (the
// gradient scatter wants the widest atomic rows); SH25: forward 4.34 / 4.04 ms, backward 13.9 / 17.8 ms for 16 / 8.
// With the forward kernel's 16-byte coefficient loads (round 2: a lane owns groups of 4 consecutive floats) the balance
// moves to fewer lanes: forward 3.51 / 2.98 / 2.44 ms for 16 / 8 / 4 lanes (dword loads: 3.88 / 3.11 / 4.23), SH25 3.45 /
// 3.06 ms for 8 / 4, SH9 2.14 ms at 4; 2 lanes measured slower again (3.25 ms).  At 4 lanes the channel-aligned ownership
// with compile-time K (KF) then takes SH16 to 1.61 ms, SH25 to 2.35 ms, SH9 to 1.75 ms.
// Backward at "4 lanes" is octree_render_bwd4_kernel (4-lane march, 16-lane cooperative scatter): 10.47 ms reusing the
// forward image / 11.20 ms without, against 10.86 / 11.90 ms for the 16-lane kernel (SH25: 14.46 / 15.49 against 14.87 / 16.02).
// So: 4 lanes both ways.  pxo_octree_set_lanes_per_ray forces a value for A/B runs and the per-instantiation tests.
static int g_row_override[2] = {0, 0};   // [forward, backward]; 0 = the measured default
static int render_row(bool backward) { return g_row_override[backward ? 1 : 0] ? g_row_override[backward ? 1 : 0] : 4; }

// Rows of the backward kernel's per-wave write-combining cache.  Measured (800x800, SH16, reusing the forward image):
// 9.7 ms direct scatter, 5.0 / 4.8 / 4.4 / 4.3 ms with 4 / 8 / 16 / 32 rows; two-march form 10.3 -> 6.3 / 6.1 / 5.6 / 6.3 (32 rows
// cost occupancy: 35 KB of LDS per workgroup).  pxo_octree_set_tuning(PXO_TUNE_BWD_CACHE_ROWS, 0 | 4 | 8 | 16 | 32 | 64)
// selects another instantiation for A/B runs (0 = direct scatter); anything else is rejected there.
static int g_bwd_wc_rows = 16;
static int g_bwd_update = 0;     // PXO_TUNE_BWD_UPDATE: 0 the whole wave on one sample's row, 1 every ray's 4 lanes on its own row

// the colour format of a tree; name: "SH" or "SG", for the message
static int check_format(int K, int data_dim, const char* name, const char* who) {
  const bool sg = name[1] == 'G';
  PXO_REQUIRE(K == 1 || K == 4 || K == 9 || K == 16 || K == 25, "%s: basis_dim %d is not %s %s format (%s1,4,9,16,25)", who, K,
              sg ? "a supported" : "an", name, sg ? "sg_dim " : "");
  PXO_REQUIRE(data_dim == 3 * K + 1, "%s: data_dim %d != 3*basis_dim+1", who, data_dim);
  return PXO_OK;
}

static int check_n_internal(int64_t n_internal, const char* who) {
  PXO_REQUIRE(n_internal >= 1 && n_internal < ((int64_t)1 << 28), "%s: n_internal out of range", who);
  return PXO_OK;
}

// the palette form (octree/compression.py:88-139) has no data_dim of its own
static int quant_format_ok(int64_t n_internal, int basis_dim, int n_retained, int bits, const char* who) {
  const int K = basis_dim;
  if (int rc = check_format(K, 3 * K + 1, "SH", who)) return rc;
  PXO_REQUIRE(n_retained >= 0 && n_retained < K, "%s: n_retained %d must be in [0, basis_dim %d)", who, n_retained, K);
  PXO_REQUIRE(bits >= 1 && bits <= 16, "%s: bits %d must be in 1..16 (the map is uint16)", who, bits);
  return check_n_internal(n_internal, who);
}

// stop_thresh < surface_thresh < 1: an early stop (light <= stop_thresh) then never comes before the crossing
static int check_surface_thresh(const PxoRenderOpts* o, float surface_thresh, const char* who) {
  PXO_REQUIRE(o->stop_thresh < surface_thresh && surface_thresh < 1.0f,
              "%s: surface_thresh %g must lie in (stop_thresh %g, 1)", who, (double)surface_thresh, (double)o->stop_thresh);
  return PXO_OK;
}

extern "C++" {   // overloads and templates

// What a tree of each form must satisfy before a renderer reads it.  lobes: non-NULL names SG in the format's message.
template <typename Tree>   // rows of float or float16
static int check_row_tree(const Tree* tree, const float* lobes, const char* who) {
  PXO_REQUIRE(tree && tree->child && tree->data, "%s: null tree", who);
  if (int rc = check_format(tree->basis_dim, tree->data_dim, lobes ? "SG" : "SH", who)) return rc;
  return check_n_internal(tree->n_internal, who);
}
static int check_tree(const PxoTree* tree, const float* lobes, const char* who) { return check_row_tree(tree, lobes, who); }
static int check_tree(const PxoHalfTree* tree, const float* lobes, const char* who) {
  if (int rc = check_row_tree(tree, lobes, who)) return rc;
  PXO_REQUIRE(tree->row_stride == ((tree->data_dim + 3) & ~3), "%s: row_stride %d is not that of pxo_octree_half_pack_bytes (%d)",
              who, tree->row_stride, (tree->data_dim + 3) & ~3);
  PXO_REQUIRE(((uintptr_t)tree->data & 7) == 0, "%s: data must be 8-byte aligned", who);
  return PXO_OK;
}
static int check_tree(const PxoQuantTree* tree, const float*, const char* who) {
  PXO_REQUIRE(tree && tree->child && tree->idx && tree->palette && tree->sigma, "%s: null tree", who);
  if (int rc = quant_format_ok(tree->n_internal, tree->basis_dim, tree->n_retained, tree->bits, who)) return rc;
  const int Kq = tree->basis_dim - tree->n_retained;
  PXO_REQUIRE(tree->idx_stride == ((Kq + 3) & ~3) && tree->ret_stride == 4 * tree->n_retained,
              "%s: strides (%d, %d) are not those of pxo_octree_quant_pack_bytes", who, tree->idx_stride, tree->ret_stride);
  PXO_REQUIRE(tree->n_retained == 0 || tree->retained, "%s: n_retained %d but retained is null", who, tree->n_retained);
  PXO_REQUIRE((((uintptr_t)tree->idx | (uintptr_t)tree->palette | (uintptr_t)tree->retained) & 7) == 0,
              "%s: idx, palette and retained must be 8-byte aligned", who);
  return PXO_OK;
}

// how a tree shades its rays: an SG tree's lobes, an NDC scene's projection (the palette form has neither)
template <typename Tree>
static void set_shading(FwdBlock<Tree>& A, const float* lobes, const PxoNdc* ndc) {
  A.lobes = lobes;
  A.ndc = ndc ? *ndc : kNoNdc;
}
static void set_shading(QuantRenderArgs&, const float*, const PxoNdc*) {}

// The argument block of every renderer launch, forward, backward and counting, of every form: the checks on the options, the
// tree (check_tree) and the rays (launch_shape), lanes per ray and block count.  The entry points check lobes and ndc first.
template <typename Block>
static int render_args(const decltype(Block::tree)* tree, const float* lobes, const PxoNdc* ndc, const PxoCamera* cam,
                       const float* origins, const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts,
                       const char* who, bool backward, Block& A, unsigned& grid, int& row) {
  if (int rc = check_opts(opts, who)) return rc;
  if (int rc = check_tree(tree, lobes, who)) return rc;
  row = render_row(backward);                    // the palette kernel is unmeasured against 8 / 16 (see DESIGN): the float default
  A.tree = *tree;
  A.opt = *opts;
  set_shading(A, lobes, ndc);
  return launch_shape(cam, origins, dirs, viewdirs, B, row, who, A, grid);
}

// Every forward entry point after its own checks of lobes and ndc.  AUX: with the alpha / depth / surface outputs.
// FOOT: with a depth per sample from the pixel footprint (cone, min_depth: already checked by check_foot).
template <typename Block, bool AUX, bool FOOT = false>
static int render_forward(const decltype(Block::tree)* tree, const float* lobes, const PxoNdc* ndc, const PxoCamera* cam,
                          const float* origins, const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts,
                          float surface_thresh, float* out_rgb, float* out_aux, void* stream, const char* who,
                          float cone = 0.0f, int min_depth = 0) {
  MaybeFoot<MaybeAux<Block, AUX>, FOOT> A;
  unsigned grid;
  int row;
  if (int rc = render_args<Block>(tree, lobes, ndc, cam, origins, dirs, viewdirs, B, opts, who, false, A, grid, row)) return rc;
  if constexpr (AUX)
    if (int rc = check_surface_thresh(opts, surface_thresh, who)) return rc;
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(out_rgb && (!AUX || out_aux), "%s: null output", who);
  if constexpr (AUX) {
    A.out = out_aux;
    A.surface_thresh = surface_thresh;
  }
  if constexpr (FOOT) {
    A.foot_g = cone * fminf(fminf(tree->invradius[0], tree->invradius[1]), tree->invradius[2]);
    A.foot_min_depth = min_depth;
  }
  launch_fwd<Block, AUX, FOOT>(A, row, grid, out_rgb, stream);
  return check_launch(who);
}

}  // extern "C++"

int pxo_octree_set_lanes_per_ray(int forward, int backward) {
  auto ok = [](int v) { return v == 0 || v == 4 || v == 8 || v == 16; };
  PXO_REQUIRE(ok(forward) && ok(backward), "pxo_octree_set_lanes_per_ray: lanes must be 0 (default), 4, 8 or 16");
  g_row_override[0] = forward;
  g_row_override[1] = backward;
  return PXO_OK;
}

int pxo_octree_set_tuning(int knob, int value) {
  switch (knob) {
    case PXO_TUNE_GW_MARCHER:
      PXO_REQUIRE(value >= -1 && value <= 1, "pxo_octree_set_tuning: marcher must be -1 (chosen on the device), 0 (per-sample) or 1 (slab-staged)");
      g_gw_marcher = value;
      return PXO_OK;
    case PXO_TUNE_BWD_CACHE_ROWS:
      PXO_REQUIRE(value == 0 || value == 4 || value == 8 || value == 16 || value == 32 || value == 64,
                  "pxo_octree_set_tuning: write-combining rows must be 0, 4, 8, 16, 32 or 64 (got %d)", value);
      g_bwd_wc_rows = value;
      return PXO_OK;
    case PXO_TUNE_GW_TILE_ORDER:
      PXO_REQUIRE(value == 0 || value == 1, "pxo_octree_set_tuning: weight-mask tile order must be 0 (linear) or 1 (XCD supertiles), got %d", value);
      g_gw_tile_order = value;
      return PXO_OK;
    case PXO_TUNE_BWD_UPDATE:
      PXO_REQUIRE(value == 0 || value == 1, "pxo_octree_set_tuning: backward update must be 0 (wave per sample) or 1 (ray-parallel), got %d", value);
      g_bwd_update = value;
      return PXO_OK;
    default:
      set_error("pxo_octree_set_tuning: unknown knob %d", knob);
      return PXO_ERR_ARG;
  }
}

int pxo_octree_get_tuning(int knob, int* value) {
  PXO_REQUIRE(value != nullptr, "pxo_octree_get_tuning: NULL pointer");
  switch (knob) {
    case PXO_TUNE_GW_MARCHER: *value = g_gw_marcher; return PXO_OK;
    case PXO_TUNE_BWD_CACHE_ROWS: *value = g_bwd_wc_rows; return PXO_OK;
    case PXO_TUNE_BWD_UPDATE: *value = g_bwd_update; return PXO_OK;
    case PXO_TUNE_GW_TILE_ORDER: *value = g_gw_tile_order; return PXO_OK;
    default: set_error("pxo_octree_get_tuning: unknown knob %d", knob); return PXO_ERR_ARG;
  }
}

// SG trees: the same launches with RenderArgs::lobes set.  The format is checked before anything else, in SG's name.
static int check_sg(const PxoTree* tree, const float* lobes, const char* who) {
  PXO_REQUIRE(tree, "%s: null tree", who);
  if (int rc = check_format(tree->basis_dim, tree->data_dim, "SG", who)) return rc;
  PXO_REQUIRE(lobes, "%s: null lobes (an SG tree needs its [basis_dim,4] extra_data)", who);
  return PXO_OK;
}

int pxo_octree_render_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                          const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream) {
  return render_forward<RenderArgs, false>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb, nullptr,
                                           stream, "pxo_octree_render_fwd");
}

int pxo_octree_render_sg_fwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                             const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb,
                             void* stream) {
  if (int rc = check_sg(tree, lobes, "pxo_octree_render_sg_fwd")) return rc;
  return render_forward<RenderArgs, false>(tree, lobes, nullptr, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb, nullptr,
                                           stream, "pxo_octree_render_sg_fwd");
}

int pxo_octree_render_aux_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                              float* out_rgb, float* out_aux, void* stream) {
  return render_forward<RenderArgs, true>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, surface_thresh, out_rgb,
                                          out_aux, stream, "pxo_octree_render_aux_fwd");
}

// ---- a depth per sample from the pixel footprint (plenoctree_octree.h, "footprint") ----
static int check_foot(const PxoTree* tree, float cone, int min_depth, const char* who) {
  PXO_REQUIRE(tree && tree->child && tree->data, "%s: null tree", who);
  PXO_REQUIRE(cone >= 0.0f && cone < INFINITY, "%s: cone %g must be finite and >= 0", who, (double)cone);
  PXO_REQUIRE(min_depth >= 0 && min_depth <= PXO_TREE_MAX_DEPTH, "%s: min_depth %d is outside [0, %d]", who, min_depth,
              PXO_TREE_MAX_DEPTH);
  return PXO_OK;
}

int pxo_octree_render_foot_fwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                               const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float cone,
                               int min_depth, float* out_rgb, void* stream) {
  const char* who = "pxo_octree_render_foot_fwd";
  if (int rc = check_foot(tree, cone, min_depth, who)) return rc;
  if (lobes)                                     // an SG tree: its format is checked in SG's name, as pxo_octree_render_sg_fwd does
    if (int rc = check_sg(tree, lobes, who)) return rc;
  return render_forward<RenderArgs, false, true>(tree, lobes, nullptr, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb,
                                                 nullptr, stream, who, cone, min_depth);
}

int pxo_octree_render_foot_aux_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                   const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float cone, int min_depth,
                                   float surface_thresh, float* out_rgb, float* out_aux, void* stream) {
  const char* who = "pxo_octree_render_foot_aux_fwd";
  if (int rc = check_foot(tree, cone, min_depth, who)) return rc;
  return render_forward<RenderArgs, true, true>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, surface_thresh,
                                                out_rgb, out_aux, stream, who, cone, min_depth);
}

static int octree_render_bwd_impl(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                  const float* viewdirs, int64_t B, const PxoRenderOpts* opts, const float* lobes,
                                  const float* out_rgb, const float* grad_out, float* grad_data, void* stream,
                                  const char* who, const PxoNdc* ndc = nullptr) {
  RenderArgs A;
  unsigned grid;
  int row;
  if (int rc = render_args(tree, lobes, ndc, cam, origins, dirs, viewdirs, B, opts, who, true, A, grid, row)) return rc;
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(grad_out && grad_data, "%s: null pointer", who);
  // the gradient pass marches exactly (no early stop, no 1/(1-T) rescale): a forward image made with
  // stop_thresh > 0 is not the image whose gradient this is
  PXO_REQUIRE(out_rgb == nullptr || opts->stop_thresh == 0.0f,
              "%s: out_rgb must come from an exact march (stop_thresh == 0), got stop_thresh %g", who,
              (double)opts->stop_thresh);
  if (row == 4) {                                // SH16 / SH25 with K a compile-time constant
    const int K = tree->basis_dim, wc = g_bwd_wc_rows;
    const bool rp = g_bwd_update == 1;
    const Bwd4Kernel kernel = K == 16 ? bwd4_kernel<16>(wc, rp) : K == 25 ? bwd4_kernel<25>(wc, rp) : bwd4_kernel<-1>(wc, rp);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRenderThreads), 0, (hipStream_t)stream, A, out_rgb, grad_out, grad_data);
  } else {
    const auto kernel = row == 8 ? octree_render_kernel<1, 8> : octree_render_kernel<1, 16>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRenderThreads), 0, (hipStream_t)stream, A, (float*)nullptr, out_rgb, grad_out,
                       grad_data);
  }
  return check_launch(who);
}

int pxo_octree_render_bwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                          const float* viewdirs, int64_t B, const PxoRenderOpts* opts, const float* out_rgb,
                          const float* grad_out, float* grad_data, void* stream) {
  return octree_render_bwd_impl(tree, cam, origins, dirs, viewdirs, B, opts, nullptr, out_rgb, grad_out, grad_data, stream,
                                "pxo_octree_render_bwd");
}

// NDC twins: every launch render_row / the PXO_TUNE_* knobs can select carries RenderArgs::ndc, so each of them runs the
// NDC set-up (none falls back to the world-space march).  check_tree checks the SH format.
int pxo_octree_render_ndc_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream,
                              const PxoNdc* ndc) {
  if (int rc = check_ndc(ndc, "pxo_octree_render_ndc_fwd")) return rc;
  return render_forward<RenderArgs, false>(tree, nullptr, ndc, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb, nullptr,
                                           stream, "pxo_octree_render_ndc_fwd");
}

int pxo_octree_render_ndc_bwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, const float* out_rgb,
                              const float* grad_out, float* grad_data, void* stream, const PxoNdc* ndc) {
  if (int rc = check_ndc(ndc, "pxo_octree_render_ndc_bwd")) return rc;
  return octree_render_bwd_impl(tree, cam, origins, dirs, viewdirs, B, opts, nullptr, out_rgb, grad_out, grad_data, stream,
                                "pxo_octree_render_ndc_bwd", ndc);
}

int pxo_octree_render_sg_bwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                             const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts,
                             const float* out_rgb, const float* grad_out, float* grad_data, void* stream) {
  if (int rc = check_sg(tree, lobes, "pxo_octree_render_sg_bwd")) return rc;
  return octree_render_bwd_impl(tree, cam, origins, dirs, viewdirs, B, opts, lobes, out_rgb, grad_out, grad_data, stream,
                                "pxo_octree_render_sg_bwd");
}

// ---- compressed trees (octree/compression.py:88-139) ----
int pxo_octree_quant_pack_bytes(int64_t n_internal, int basis_dim, int n_retained, int bits, PxoQuantLayout* layout) {
  if (int rc = quant_format_ok(n_internal, basis_dim, n_retained, bits, "pxo_octree_quant_pack_bytes")) return rc;
  PXO_REQUIRE(layout, "pxo_octree_quant_pack_bytes: null layout");
  const int64_t cells = n_internal * 8, Kq = basis_dim - n_retained;
  PxoQuantLayout L{};
  L.idx_stride = (int32_t)((Kq + 3) & ~(int64_t)3);
  L.ret_stride = 4 * n_retained;
  int64_t off = 0;
  L.idx_offset = off;      off += align256(cells * L.idx_stride * 2);
  L.palette_offset = off;  off += align256((Kq << bits) * 8);
  L.sigma_offset = off;    off += align256(cells * 4);
  L.retained_offset = off; off += align256(cells * L.ret_stride * 2);
  L.total_bytes = off;
  *layout = L;
  return PXO_OK;
}

int pxo_octree_quant_pack(const uint16_t* quant_map, const void* quant_colors, const void* sigma, int sigma_elem_bytes,
                          const void* data_retained, int64_t n_internal, int basis_dim, int n_retained, int bits,
                          void* packed, size_t packed_bytes, void* stream) {
  PxoQuantLayout L;
  if (int rc = pxo_octree_quant_pack_bytes(n_internal, basis_dim, n_retained, bits, &L)) return rc;
  PXO_REQUIRE(quant_map && quant_colors && sigma && packed, "pxo_octree_quant_pack: null pointer");
  PXO_REQUIRE(n_retained == 0 || data_retained, "pxo_octree_quant_pack: n_retained %d but data_retained is null", n_retained);
  PXO_REQUIRE(sigma_elem_bytes == 2 || sigma_elem_bytes == 4, "pxo_octree_quant_pack: sigma must be float16 (2) or float32 (4)");
  PXO_REQUIRE(((uintptr_t)packed & 255) == 0, "pxo_octree_quant_pack: packed buffer must be 256-byte aligned");
  if (packed_bytes < (size_t)L.total_bytes) {
    set_error("pxo_octree_quant_pack: buffer %zu < %lld", packed_bytes, (long long)L.total_bytes);
    return PXO_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(packed);
  const int64_t cells = n_internal * 8;
  const int Kq = basis_dim - n_retained, groups = L.idx_stride / 4;
  hipLaunchKernelGGL(quant_pack_idx_kernel, dim3((unsigned)blocks_for(cells * groups, 256)), dim3(256), 0, s, quant_map, cells, Kq,
                     groups, reinterpret_cast<u16x4*>(base + L.idx_offset));
  const int64_t entries = (int64_t)Kq << bits;
  hipLaunchKernelGGL(quant_pack_pad_kernel, dim3((unsigned)blocks_for(entries, 256)), dim3(256), 0, s,
                     static_cast<const _Float16*>(quant_colors), entries, reinterpret_cast<f16x4*>(base + L.palette_offset));
  float* sig = reinterpret_cast<float*>(base + L.sigma_offset);
  if (sigma_elem_bytes == 2)
    hipLaunchKernelGGL(quant_pack_sigma_kernel<_Float16>, dim3((unsigned)blocks_for(cells, 256)), dim3(256), 0, s,
                       static_cast<const _Float16*>(sigma), cells, sig);
  else
    hipLaunchKernelGGL(quant_pack_sigma_kernel<float>, dim3((unsigned)blocks_for(cells, 256)), dim3(256), 0, s,
                       static_cast<const float*>(sigma), cells, sig);
  if (n_retained)
    hipLaunchKernelGGL(quant_pack_retained_kernel, dim3((unsigned)blocks_for(cells * n_retained, 256)), dim3(256), 0, s,
                       static_cast<const _Float16*>(data_retained), cells, n_retained,
                       reinterpret_cast<f16x4*>(base + L.retained_offset));
  return check_launch("octree_quant_pack");
}

int pxo_octree_render_quant_fwd(const PxoQuantTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream) {
  return render_forward<QuantRenderArgs, false>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb,
                                                nullptr, stream, "pxo_octree_render_quant_fwd");
}

int pxo_octree_render_quant_aux_fwd(const PxoQuantTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                    const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                                    float* out_rgb, float* out_aux, void* stream) {
  return render_forward<QuantRenderArgs, true>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, surface_thresh,
                                               out_rgb, out_aux, stream, "pxo_octree_render_quant_aux_fwd");
}

// ---- float16 trees rendered in place (the data array of the files N3Tree.save writes) ----
static int half_format_ok(int64_t n_internal, int data_dim, const char* who) {
  PXO_REQUIRE(data_dim >= 4 && (data_dim - 1) % 3 == 0, "%s: data_dim %d is not 3*basis_dim+1", who, data_dim);
  if (int rc = check_format((data_dim - 1) / 3, data_dim, "SH", who)) return rc;
  return check_n_internal(n_internal, who);
}

int pxo_octree_half_pack_bytes(int64_t n_internal, int data_dim, int32_t* row_stride, int64_t* bytes) {
  if (int rc = half_format_ok(n_internal, data_dim, "pxo_octree_half_pack_bytes")) return rc;
  PXO_REQUIRE(row_stride && bytes, "pxo_octree_half_pack_bytes: null output");
  *row_stride = (data_dim + 3) & ~3;
  *bytes = n_internal * 8 * *row_stride * 2;
  return PXO_OK;
}

int pxo_octree_half_pack(const void* src, int64_t n_internal, int data_dim, void* packed, size_t packed_bytes, void* stream) {
  int32_t row_stride;
  int64_t bytes;
  if (int rc = pxo_octree_half_pack_bytes(n_internal, data_dim, &row_stride, &bytes)) return rc;
  PXO_REQUIRE(src && packed, "pxo_octree_half_pack: null pointer");
  PXO_REQUIRE(((uintptr_t)packed & 7) == 0, "pxo_octree_half_pack: packed buffer must be 8-byte aligned");
  if (packed_bytes < (size_t)bytes) {
    set_error("pxo_octree_half_pack: buffer %zu < %lld", packed_bytes, (long long)bytes);
    return PXO_ERR_WORKSPACE;
  }
  const int64_t cells = n_internal * 8;          // < 2^31 cells x at most 76 halves: fewer than 2^31 blocks of 256
  hipLaunchKernelGGL(half_pack_kernel, dim3((unsigned)blocks_for(cells * row_stride, 256)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const _Float16*>(src), cells, data_dim, (int)row_stride, static_cast<_Float16*>(packed));
  return check_launch("octree_half_pack");
}

int pxo_octree_render_half_fwd(const PxoHalfTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                               const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb,
                               void* stream, const PxoNdc* ndc) {
  const char* who = "pxo_octree_render_half_fwd";
  PXO_REQUIRE(!(lobes && ndc), "%s: SG trees have no NDC form (lobes and ndc are both set)", who);
  if (ndc)
    if (int rc = check_ndc(ndc, who)) return rc;
  return render_forward<FwdBlock<PxoHalfTree>, false>(tree, lobes, ndc, cam, origins, dirs, viewdirs, B, opts, 0.0f, out_rgb,
                                                      nullptr, stream, who);
}

int pxo_octree_render_half_aux_fwd(const PxoHalfTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                   const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                                   float* out_rgb, float* out_aux, void* stream) {
  return render_forward<FwdBlock<PxoHalfTree>, true>(tree, nullptr, nullptr, cam, origins, dirs, viewdirs, B, opts, surface_thresh,
                                                     out_rgb, out_aux, stream, "pxo_octree_render_half_aux_fwd");
}

int pxo_octree_count_work(const PxoTree* tree, const PxoCamera* cam, const PxoRenderOpts* opts, unsigned long long* counts,
                          uint8_t* leaf_seen, void* stream) {
  const char* who = "pxo_octree_count_work";
  PXO_REQUIRE(cam != nullptr && counts != nullptr, "%s: needs a camera and a counts[4] buffer", who);
  RenderArgs A;
  unsigned grid;
  int row;
  const int64_t rays = (int64_t)cam->width * cam->height;
  if (int rc = render_args(tree, nullptr, nullptr, cam, nullptr, nullptr, nullptr, rays, opts, who, false, A, grid, row)) return rc;
  hipLaunchKernelGGL(octree_count_kernel, dim3((unsigned)blocks_for(rays, 256)), dim3(256), 0, (hipStream_t)stream, A, counts,
                     leaf_seen);
  return check_launch(who);
}

// what the two weight entry points share: the checks on tree / options / ndc / weights and the launch (op: checked by the
// entry points, ahead of their no-work return)
static int weight_accum_launch(const PxoTree* tree, WeightArgs& A, const PxoRenderOpts* opts, int op, float* weights,
                               void* stream, const PxoNdc* ndc, const char* who) {
  if (int rc = check_opts(opts, who)) return rc;
  PXO_REQUIRE(tree && tree->child && tree->data, "%s: null tree", who);
  PXO_REQUIRE(tree->data_dim >= 1, "%s: data_dim %d < 1", who, tree->data_dim);
  if (int rc = check_n_internal(tree->n_internal, who)) return rc;
  PXO_REQUIRE(weights, "%s: null weights", who);
  if (ndc)
    if (int rc = check_ndc(ndc, who)) return rc;
  const int64_t blocks = blocks_for(A.n_rays, 256);
  PXO_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many rays for one launch", who);
  A.tree = *tree;
  A.opt = *opts;
  A.ndc = ndc ? *ndc : kNoNdc;
  A.weights = weights;
  if (op == 0)
    hipLaunchKernelGGL(octree_weight_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(octree_weight_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
  return check_launch(who);
}

int pxo_octree_weight_accum_cams(const PxoTree* tree, const float* c2w_all, int n_cams, float fx, float fy, int width,
                                 int height, const PxoRenderOpts* opts, int op, float* weights, void* stream,
                                 const PxoNdc* ndc) {
  const char* who = "pxo_octree_weight_accum_cams";
  PXO_REQUIRE(op == 0 || op == 1, "%s: op %d is neither 0 (max) nor 1 (sum)", who, op);
  PXO_REQUIRE(n_cams >= 0, "%s: n_cams %d < 0", who, n_cams);
  PXO_REQUIRE(width >= 1 && height >= 1 && fx > 0.0f && fy > 0.0f, "%s: bad camera (width, height >= 1, focal lengths > 0)", who);
  if (n_cams == 0) return PXO_OK;
  PXO_REQUIRE(c2w_all, "%s: null c2w_all", who);
  WeightArgs A{};
  A.c2w_all = c2w_all;
  A.fx = fx; A.fy = fy; A.W = width; A.H = height;
  A.n_rays = (int64_t)n_cams * width * height;
  return weight_accum_launch(tree, A, opts, op, weights, stream, ndc, who);
}

int pxo_octree_weight_accum_rays(const PxoTree* tree, const float* origins, const float* dirs, int64_t B,
                                 const PxoRenderOpts* opts, int op, float* weights, void* stream, const PxoNdc* ndc) {
  const char* who = "pxo_octree_weight_accum_rays";
  PXO_REQUIRE(op == 0 || op == 1, "%s: op %d is neither 0 (max) nor 1 (sum)", who, op);
  PXO_REQUIRE(B >= 0, "%s: B < 0", who);
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(origins && dirs, "%s: null ray arrays", who);
  WeightArgs A{};
  A.origins = origins; A.dirs = dirs;
  A.n_rays = B;
  return weight_accum_launch(tree, A, opts, op, weights, stream, ndc, who);
}

int pxo_tree_collapse_mark(const int32_t* child, const int32_t* parent_depth, const uint8_t* keep, int64_t n, int max_depth,
                           uint8_t* node_dead, void* stream) {
  PXO_REQUIRE(n >= 1 && n < ((int64_t)1 << 28), "pxo_tree_collapse_mark: n out of range");
  PXO_REQUIRE(max_depth >= 0 && max_depth <= kMaxD, "pxo_tree_collapse_mark: max_depth %d outside [0, %d]", max_depth, kMaxD);
  PXO_REQUIRE(child && parent_depth && keep && node_dead, "pxo_tree_collapse_mark: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(node_dead, 0, (size_t)n, s) != hipSuccess) {      // the root (depth 0) is never removed
    set_error("pxo_tree_collapse_mark: hipMemsetAsync failed");
    return PXO_ERR_HIP;
  }
  for (int d = max_depth; d >= 1; --d)
    hipLaunchKernelGGL(tree_collapse_mark_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, s, child, parent_depth, keep,
                       n, d, node_dead);
  return check_launch("tree_collapse_mark");
}

int pxo_tree_collapse_emit(const int32_t* child, const int32_t* parent_depth, const float* data, int data_dim,
                           const uint8_t* keep, const uint8_t* node_dead, const int64_t* new_index, int64_t n, int64_t n_new,
                           int32_t* new_child, int32_t* new_parent_depth, float* new_data, int64_t* old2new, void* stream) {
  PXO_REQUIRE(n >= 1 && n < ((int64_t)1 << 28) && n_new >= 1 && n_new <= n, "pxo_tree_collapse_emit: n / n_new out of range");
  PXO_REQUIRE(data_dim >= 1 && data_dim <= 256, "pxo_tree_collapse_emit: data_dim %d outside [1, 256]", data_dim);
  PXO_REQUIRE(child && parent_depth && data && keep && node_dead && new_index && new_child && new_parent_depth && new_data &&
              old2new, "pxo_tree_collapse_emit: null pointer");
  const int64_t data_blocks = blocks_for(n * 8 * data_dim, 256);
  PXO_REQUIRE(data_blocks < ((int64_t)1 << 31), "pxo_tree_collapse_emit: too many data elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tree_collapse_struct_kernel, dim3((unsigned)blocks_for(n * 8, 256)), dim3(256), 0, s, child, parent_depth,
                     node_dead, new_index, n, new_child, new_parent_depth, old2new);
  hipLaunchKernelGGL(tree_collapse_data_kernel, dim3((unsigned)data_blocks), dim3(256), 0, s, child, data, data_dim, keep,
                     node_dead, new_index, n, new_data);
  return check_launch("tree_collapse_emit");
}

int pxo_grid_weight_count_work(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                               int width, int height, const PxoRenderOpts* opts, const float offset[3],
                               const float invradius[3], unsigned long long* counts, uint8_t* voxel_seen, void* stream) {
  if (int rc = check_opts(opts, "pxo_grid_weight_count_work")) return rc;
  PXO_REQUIRE(sigma_grid && c2w_all && offset && invradius && counts && reso >= 1 && n_cams >= 1 && width >= 1 && height >= 1,
              "pxo_grid_weight_count_work: bad arguments");
  // the counting march divides by the grid size as the power-of-two weight-mask kernels do (an exact multiplication); for
  // other sizes the renderer's own step arithmetic differs in the last bit and the counted sample sequence could too
  PXO_REQUIRE((reso & (reso - 1)) == 0 && reso >= 4, "pxo_grid_weight_count_work: reso %d is not a power of two >= 4 "
              "(the counters repeat the march of the power-of-two weight-mask kernels only)", reso);
  Vec3 o, ir;
  for (int a = 0; a < 3; ++a) { o.v[a] = offset[a]; ir.v[a] = invradius[a]; }
  const int64_t rays = (int64_t)width * height * n_cams;
  hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)blocks_for(rays, 256)), dim3(256), 0, (hipStream_t)stream, sigma_grid, reso,
                     c2w_all, n_cams, fx, fy, width, height, *opts, o, ir, counts, voxel_seen);
  return check_launch("grid_weight_count_work");
}

// ---- scene (plenoctree_octree.h, "scene") ----
static int check_scene_n(int n, const char* who) {
  PXO_REQUIRE(n >= 1 && n <= PXO_SCENE_MAX_INSTANCES, "%s: %d instances, a scene takes 1 .. %d", who, n, PXO_SCENE_MAX_INSTANCES);
  return PXO_OK;
}

int pxo_scene_lds_bytes(int n, size_t* bytes) {
  if (int rc = check_scene_n(n, "pxo_scene_lds_bytes")) return rc;
  PXO_REQUIRE(bytes, "pxo_scene_lds_bytes: null pointer");
  *bytes = (size_t)n * kSceneRays * kSceneWordsPerRay * sizeof(int);
  return PXO_OK;
}

int pxo_scene_check(const PxoInstance* instances, int n) {
  const char* who = "pxo_scene_check";
  if (int rc = check_scene_n(n, who)) return rc;
  PXO_REQUIRE(instances, "%s: null instances", who);
  for (int i = 0; i < n; ++i) {
    const PxoInstance& I = instances[i];
    if (int rc = check_tree(&I.tree, nullptr, who)) return rc;
    PXO_REQUIRE(I.scale > 0.0f && I.scale < INFINITY, "%s: instance %d: scale %g must be finite and > 0", who, i, (double)I.scale);
    PXO_REQUIRE(I.inv_scale == 1.0f / I.scale, "%s: instance %d: inv_scale %g is not 1 / scale", who, i, (double)I.inv_scale);
    bool finite = true;
    for (int k = 0; k < 9; ++k) finite = finite && fabsf(I.rot_t[k]) < INFINITY;
    for (int k = 0; k < 3; ++k) finite = finite && fabsf(I.trans[k]) < INFINITY;
    PXO_REQUIRE(finite, "%s: instance %d: rot_t / trans must be finite", who, i);
  }
  return PXO_OK;
}

int pxo_scene_render_fwd(const PxoInstance* d_instances, int n, const PxoCamera* cam, const float* origins, const float* dirs,
                         const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream) {
  const char* who = "pxo_scene_render_fwd";
  if (int rc = check_scene_n(n, who)) return rc;
  PXO_REQUIRE(d_instances, "%s: null instances", who);
  if (int rc = check_opts(opts, who)) return rc;
  SceneArgs A;
  unsigned grid;
  if (int rc = launch_shape(cam, origins, dirs, viewdirs, B, kSceneRow, who, A, grid)) return rc;
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(out_rgb, "%s: null output", who);
  A.inst = d_instances;
  A.n = n;
  A.opt = *opts;
  const size_t lds = (size_t)n * kSceneRays * kSceneWordsPerRay * sizeof(int);
  // more than 64 KB of dynamic LDS (5 instances and up) has to be allowed per function and device; a host-side setting
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(scene_render_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess) {
    set_error("%s: %zu bytes of LDS for %d instances refused by the device", who, lds, n);
    return PXO_ERR_HIP;
  }
  hipLaunchKernelGGL(scene_render_kernel, dim3(grid), dim3(kRenderThreads), lds, (hipStream_t)stream, A, out_rgb);
  return check_launch(who);
}

int pxo_image_mse(const float* im, const float* gt, int64_t n, float* grad, float* sse_out, void* stream) {
  PXO_REQUIRE(n >= 1, "pxo_image_mse: n < 1");
  PXO_REQUIRE(im && gt && sse_out, "pxo_image_mse: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(sse_out, 0, sizeof(float), s) != hipSuccess) {
    set_error("pxo_image_mse: hipMemsetAsync failed");
    return PXO_ERR_HIP;
  }
  const int64_t blocks = blocks_for(n, kMseBlock * kMsePerThread);
  hipLaunchKernelGGL(image_mse_kernel, dim3((unsigned)(blocks > kMseMaxBlocks ? kMseMaxBlocks : blocks)), dim3(kMseBlock), 0, s, im, gt, n,
                     grad, sse_out);
  return check_launch("image_mse");
}

int pxo_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float mu, int nesterov,
                 int first_step, void* stream) {
  PXO_REQUIRE(n >= 0, "pxo_sgd_step: n < 0");
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(params && grads, "pxo_sgd_step: null pointer");
  PXO_REQUIRE(mu == 0.0f || momentum_buf, "pxo_sgd_step: momentum needs a buffer");
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, params, grads,
                     momentum_buf, n, lr, mu, nesterov, first_step);
  return check_launch("sgd_step");
}

}  // extern "C"
