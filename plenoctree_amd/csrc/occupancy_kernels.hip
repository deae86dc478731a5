// Occupancy grid of the NeRF ray renderer (gfx950): a bit per cell of a dense grid over the scene's box, and the three passes
// that let pxo_render_fwd_culled (pxo_api.hip) send only the samples in occupied cells through the fused MLP.  Entry points:
// pxo_occ_pack / pxo_occ_cull_workspace_bytes / pxo_occ_cull / pxo_occ_expand (include/plenoctree_hip.h, "occupancy grid").
// No reference counterpart: the reference evaluates every sample of every ray (nerf_sh/nerf/models.py:242-264, :308-330).
//
//   pack     sigma [reso^3] -> bits: one lane per output word, 32 cells each, the (2 dilate + 1)^3 neighbourhood clipped to the grid
//   cull     classify (one point per lane: live flag, per-block count) -> exclusive scan of the block counts (tile sums, one
//            workgroup over the tile sums, every tile in place) -> emit (rank inside the wave from a ballot, wave totals through
//            LDS, block offset from the scan): slot[] and the live points in their original order.  No atomics: two calls give
//            the same bits.  The structure is that of the marching cubes' count / emit passes (mesh_kernels.hip).
//   expand   the gather that puts the MLP's compact rows back: dense row m copies compact row slot[m], or is zero
//   gather   its inverse for the reverse pass of pxo_train_fwd_bwd_culled: dense row m goes to compact row slot[m], or is dropped
#include "pxo_common.h"

namespace pxo {

constexpr int kOccBlock = 256;        // points per workgroup (4 waves, one point per lane)
constexpr int kOccWaves = kOccBlock / 64;
constexpr int kOccScanTile = 1024;    // block counts per scan tile (256 threads x 4)

// workspace of one cull over M points (bytes, every section 256-byte aligned); nb = ceil(M / kOccBlock), nt = ceil(nb / kOccScanTile)
//   flags  uint8 [M]      1 = live
//   bsum   uint32 [nb]    live points per block, scanned in place to exclusive block offsets
//   tsum   int64 [nt]     tile sums, scanned in place to exclusive tile offsets
struct OccWs { int64_t nb, nt, flag_off, bsum_off, tsum_off, total; };

static OccWs occ_ws(int64_t M) {
  OccWs w{};
  w.nb = (M + kOccBlock - 1) / kOccBlock;
  w.nt = (w.nb + kOccScanTile - 1) / kOccScanTile;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off += (bytes + 255) & ~(int64_t)255; return o; };
  w.flag_off = take(M);
  w.bsum_off = take(4 * w.nb);
  w.tsum_off = take(8 * w.nt);
  w.total = off;
  return w;
}

size_t occ_cull_workspace_bytes(int64_t M) { return (size_t)occ_ws(M > 0 ? M : 1).total; }

// the grid as the kernels take it (by value: no device copy of the caller's struct)
struct OccView {
  const uint32_t* bits;
  int reso;
  float reso_f;
  float off[3], sc[3];
  int outside_live;
};

int occ_validate(const PxoOccGrid* occ, const char* who) {
  PXO_REQUIRE(occ != nullptr, "%s: occ is NULL", who);
  PXO_REQUIRE(occ->bits != nullptr, "%s: occ->bits is NULL", who);
  PXO_REQUIRE(occ->reso >= 1 && occ->reso <= PXO_OCC_MAX_RESO, "%s: occ->reso %d outside [1,%d]", who, occ->reso, PXO_OCC_MAX_RESO);
  for (int a = 0; a < 3; ++a) {
    const float sc = occ->scale[a];
    PXO_REQUIRE(sc == sc && sc - sc == 0.f && sc != 0.f, "%s: occ->scale[%d] = %g is zero or not finite", who, a, (double)sc);
  }
  PXO_REQUIRE(occ->outside_live == 0 || occ->outside_live == 1, "%s: occ->outside_live %d is not 0 / 1", who, occ->outside_live);
  return PXO_OK;
}

static OccView occ_view(const PxoOccGrid& g) {
  OccView v;
  v.bits = g.bits;
  v.reso = g.reso;
  v.reso_f = (float)g.reso;
  for (int a = 0; a < 3; ++a) { v.off[a] = g.offset[a]; v.sc[a] = g.scale[a]; }
  v.outside_live = g.outside_live;
  return v;
}

__device__ inline int occ_lane() { return threadIdx.x & 63; }
__device__ inline int occ_wave() { return threadIdx.x >> 6; }

__device__ inline bool occ_finite(float x) { return x - x == 0.f; }

// ---- pack ------------------------------------------------------------------------------------------------------------------
// n = reso^3 <= 2^30 cells: every index fits 32 bits
__global__ __launch_bounds__(256) void occ_pack_kernel(const float* __restrict__ sigma, int reso, uint32_t n, float thresh,
                                                       int dilate, uint32_t* __restrict__ bits, uint32_t nwords) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= nwords) return;
  const uint32_t c0 = w * 32u, r = (uint32_t)reso;
  const uint32_t q = c0 / r;
  int z = (int)(c0 - q * r), x = (int)(q / r);
  int y = (int)(q - (uint32_t)x * r);
  uint32_t word = 0;
  for (int b = 0; b < 32 && c0 + (uint32_t)b < n; ++b) {
    bool occ = false;
    const int x0 = max(x - dilate, 0), x1 = min(x + dilate, reso - 1);
    const int y0 = max(y - dilate, 0), y1 = min(y + dilate, reso - 1);
    const int z0 = max(z - dilate, 0), z1 = min(z + dilate, reso - 1);
    for (int xx = x0; xx <= x1; ++xx)
      for (int yy = y0; yy <= y1; ++yy)
        for (int zz = z0; zz <= z1; ++zz)
          occ |= !(sigma[((uint32_t)xx * r + (uint32_t)yy) * r + (uint32_t)zz] <= thresh);      // a NaN sigma is occupied
    word |= (uint32_t)occ << b;
    if (++z == reso) { z = 0; if (++y == reso) { y = 0; ++x; } }
  }
  bits[w] = word;
}

// ---- cull ------------------------------------------------------------------------------------------------------------------
__device__ inline bool occ_live(const OccView& g, float px, float py, float pz) {
  if (!(occ_finite(px) && occ_finite(py) && occ_finite(pz))) return true;      // a broken input stays visible in the image
  const float tx = fmaf(px, g.sc[0], g.off[0]), ty = fmaf(py, g.sc[1], g.off[1]), tz = fmaf(pz, g.sc[2], g.off[2]);
  const bool inside = tx >= 0.f && tx < 1.f && ty >= 0.f && ty < 1.f && tz >= 0.f && tz < 1.f;
  if (!inside) return g.outside_live != 0;
  const int last = g.reso - 1;
  const uint32_t cx = (uint32_t)min((int)(tx * g.reso_f), last), cy = (uint32_t)min((int)(ty * g.reso_f), last),
                 cz = (uint32_t)min((int)(tz * g.reso_f), last);
  const uint32_t i = (cx * (uint32_t)g.reso + cy) * (uint32_t)g.reso + cz;
  return (g.bits[i >> 5] >> (i & 31u)) & 1u;
}

__global__ __launch_bounds__(kOccBlock) void occ_classify_kernel(OccView g, const float* __restrict__ pts, int64_t M,
                                                                 uint8_t* __restrict__ flags, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t wsum[kOccWaves];
  const int64_t m = blockIdx.x * (int64_t)kOccBlock + threadIdx.x;
  bool live = false;
  if (m < M) {
    live = occ_live(g, pts[3 * m], pts[3 * m + 1], pts[3 * m + 2]);
    flags[m] = (uint8_t)live;
  }
  const uint64_t b = __ballot(live);
  if (occ_lane() == 0) wsum[occ_wave()] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kOccWaves; ++w) s += wsum[w];
    bsum[blockIdx.x] = s;
  }
}

// inclusive scans over the 64 lanes of a wave
__device__ inline uint32_t occ_wave_scan(uint32_t v) {
  const int lane = occ_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}
__device__ inline int64_t occ_wave_scan64(int64_t v) {
  const int lane = occ_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// grid nt: tsum[tile] = sum of the tile's block counts
__global__ __launch_bounds__(256) void occ_tile_sum_kernel(const uint32_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ tsum) {
  __shared__ uint32_t wsum[4];
  const int64_t i0 = blockIdx.x * (int64_t)kOccScanTile + threadIdx.x * 4;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < nb) s += bsum[i0 + k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (occ_lane() == 0) wsum[occ_wave()] = s;
  __syncthreads();
  if (threadIdx.x == 0) tsum[blockIdx.x] = (int64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one wave: exclusive scan of the tile sums in place, and the total
__global__ __launch_bounds__(64) void occ_tile_scan_kernel(int64_t* __restrict__ tsum, int64_t nt, int64_t* __restrict__ n_live) {
  const int lane = occ_lane();
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < nt; i0 += 64) {
    const int64_t i = i0 + lane;
    const int64_t v = i < nt ? tsum[i] : 0;
    const int64_t incl = occ_wave_scan64(v);
    if (i < nt) tsum[i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) *n_live = carry;
}

// grid nt: exclusive scan of a tile's block counts in place, offset by the tile's own exclusive offset (M < 2^31: 32 bits hold it)
__global__ __launch_bounds__(256) void occ_block_scan_kernel(uint32_t* __restrict__ bsum, int64_t nb, const int64_t* __restrict__ tsum) {
  __shared__ uint32_t wsum[4];
  const int64_t i0 = blockIdx.x * (int64_t)kOccScanTile + threadIdx.x * 4;
  uint32_t v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = i0 + k < nb ? bsum[i0 + k] : 0u;
    s += v[k];
  }
  const uint32_t incl = occ_wave_scan(s);
  if (occ_lane() == 63) wsum[occ_wave()] = incl;
  __syncthreads();
  uint32_t off = (uint32_t)tsum[blockIdx.x] + incl - s;
  for (int w = 0; w < occ_wave(); ++w) off += wsum[w];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < nb) bsum[i0 + k] = off;
    off += v[k];
  }
}

__global__ __launch_bounds__(kOccBlock) void occ_emit_kernel(const float* __restrict__ pts, int64_t M, const uint8_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ boff, float* __restrict__ pts_live,
                                                             int32_t* __restrict__ slot) {
  __shared__ uint32_t wsum[kOccWaves];
  const int64_t m = blockIdx.x * (int64_t)kOccBlock + threadIdx.x;
  const bool live = m < M && flags[m] != 0;
  const int lane = occ_lane(), wave = occ_wave();
  const uint64_t b = __ballot(live);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (m >= M) return;
  uint32_t off = boff[blockIdx.x] + (uint32_t)__popcll(b & (((uint64_t)1 << lane) - 1));
  for (int w = 0; w < wave; ++w) off += wsum[w];
  slot[m] = live ? (int32_t)off : -1;
  if (live) {                                         // off < the number of live points <= M: inside pts_live [n_live, 3]
    pts_live[3 * (int64_t)off] = pts[3 * m];
    pts_live[3 * (int64_t)off + 1] = pts[3 * m + 1];
    pts_live[3 * (int64_t)off + 2] = pts[3 * m + 2];
  }
}

// ---- expand ----------------------------------------------------------------------------------------------------------------
// A workgroup writes kExpandPerBlock consecutive elements of raw_rgb [M,C], a lane every 256th of them (consecutive lanes,
// consecutive addresses); the lane of a row's first channel also writes the row's sigma.  CT > 0: the width is a compile-time constant (the five SH / SG head widths 3 (deg+1)^2), so the two divisions
// are multiplications (142 -> 125 us for 1.57 M rows of 48 channels, 50 us of HBM time); CT = 0 is the general form.
constexpr int kExpandPerBlock = 1024;      // elements per workgroup: 4 per lane, 256 lanes apart (a workgroup per 256 is launch-bound)
template <int CT>
__global__ __launch_bounds__(256) void occ_expand_kernel(const float* __restrict__ rgb_live, const float* __restrict__ sigma_live,
                                                         const int32_t* __restrict__ slot, int64_t M, uint32_t c_runtime,
                                                         float* __restrict__ raw_rgb, float* __restrict__ raw_sigma) {
  const uint32_t C = CT > 0 ? (uint32_t)CT : c_runtime;
  const int64_t e0 = blockIdx.x * (int64_t)kExpandPerBlock;
  const int64_t m0 = e0 / C;
  const uint32_t l0 = (uint32_t)(e0 - m0 * C) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kExpandPerBlock / 256; ++k) {
    const uint32_t l = l0 + 256u * k;
    const uint32_t dm = l / C, c = l - dm * C;
    const int64_t m = m0 + dm;
    if (m >= M) return;                               // rows only grow with k
    const int32_t s = slot[m];
    raw_rgb[m * C + c] = s >= 0 ? rgb_live[(int64_t)s * C + c] : 0.f;
    if (c == 0) raw_sigma[m] = s >= 0 ? sigma_live[s] : 0.f;
  }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
// occ_expand_kernel's shape the other way round: a lane per element of the DENSE d_raw_rgb [M,C] (consecutive lanes, consecutive
// addresses on the read side, and on the write side inside every run of live rows, whose slots are consecutive); the element
// of a live row goes to compact row slot[m], the lane of a row's first channel also moves the row's d_sigma.  The live rows'
// slots are distinct: every compact element has one writer.  A slot outside [0, M) is dropped (the compact arrays hold M rows).
template <int CT>
__global__ __launch_bounds__(256) void occ_gather_kernel(const float* __restrict__ d_rgb, const float* __restrict__ d_sigma,
                                                         const int32_t* __restrict__ slot, int64_t M, uint32_t c_runtime,
                                                         float* __restrict__ d_rgb_live, float* __restrict__ d_sigma_live) {
  const uint32_t C = CT > 0 ? (uint32_t)CT : c_runtime;
  const int64_t e0 = blockIdx.x * (int64_t)kExpandPerBlock;
  const int64_t m0 = e0 / C;
  const uint32_t l0 = (uint32_t)(e0 - m0 * C) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kExpandPerBlock / 256; ++k) {
    const uint32_t l = l0 + 256u * k;
    const uint32_t dm = l / C, c = l - dm * C;
    const int64_t m = m0 + dm;
    if (m >= M) return;                               // rows only grow with k
    const int32_t s = slot[m];
    if (s < 0 || (int64_t)s >= M) continue;
    d_rgb_live[(int64_t)s * C + c] = d_rgb[m * C + c];
    if (c == 0) d_sigma_live[s] = d_sigma[m];
  }
}

// slot[i] = first + i for the n rows that are live whatever the grid says (the sparsity points behind the last level's samples)
__global__ __launch_bounds__(256) void occ_tail_slots_kernel(int32_t* __restrict__ slot, int64_t n, int32_t first) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < n) slot[i] = first + (int32_t)i;
}

// ---- launchers (also used by pxo_render_fwd_culled) ------------------------------------------------------------------------
int launch_occ_cull(const PxoOccGrid& occ, const float* pts, int64_t M, float* pts_live, int32_t* slot, int64_t* n_live_dev,
                    void* ws, hipStream_t s) {
  const OccWs w = occ_ws(M);
  char* base = (char*)ws;
  uint8_t* flags = (uint8_t*)(base + w.flag_off);
  uint32_t* bsum = (uint32_t*)(base + w.bsum_off);
  int64_t* tsum = (int64_t*)(base + w.tsum_off);
  hipLaunchKernelGGL(occ_classify_kernel, dim3((unsigned)w.nb), dim3(kOccBlock), 0, s, occ_view(occ), pts, M, flags, bsum);
  hipLaunchKernelGGL(occ_tile_sum_kernel, dim3((unsigned)w.nt), dim3(256), 0, s, (const uint32_t*)bsum, w.nb, tsum);
  hipLaunchKernelGGL(occ_tile_scan_kernel, dim3(1), dim3(64), 0, s, tsum, w.nt, n_live_dev);
  hipLaunchKernelGGL(occ_block_scan_kernel, dim3((unsigned)w.nt), dim3(256), 0, s, bsum, w.nb, (const int64_t*)tsum);
  hipLaunchKernelGGL(occ_emit_kernel, dim3((unsigned)w.nb), dim3(kOccBlock), 0, s, pts, M, (const uint8_t*)flags,
                     (const uint32_t*)bsum, pts_live, slot);
  return check_launch("occ_cull");
}

int launch_occ_expand(const float* rgb_live, const float* sigma_live, const int32_t* slot, int64_t M, int C, float* raw_rgb,
                      float* raw_sigma, hipStream_t s) {
  const int64_t blocks = (M * C + kExpandPerBlock - 1) / kExpandPerBlock;
  const dim3 grid((unsigned)blocks), block(256);
  switch (C) {
#define PXO_EXPAND_CASE(CT)                                                                                                       \
    case CT: hipLaunchKernelGGL(occ_expand_kernel<CT>, grid, block, 0, s, rgb_live, sigma_live, slot, M, (uint32_t)C, raw_rgb, raw_sigma); \
      break;
    PXO_EXPAND_CASE(3) PXO_EXPAND_CASE(12) PXO_EXPAND_CASE(27) PXO_EXPAND_CASE(48) PXO_EXPAND_CASE(75)
#undef PXO_EXPAND_CASE
    default: hipLaunchKernelGGL(occ_expand_kernel<0>, grid, block, 0, s, rgb_live, sigma_live, slot, M, (uint32_t)C, raw_rgb, raw_sigma);
  }
  return check_launch("occ_expand");
}

int launch_occ_gather(const float* d_rgb, const float* d_sigma, const int32_t* slot, int64_t M, int C, float* d_rgb_live,
                      float* d_sigma_live, hipStream_t s) {
  const int64_t blocks = (M * C + kExpandPerBlock - 1) / kExpandPerBlock;
  const dim3 grid((unsigned)blocks), block(256);
  switch (C) {
#define PXO_GATHER_CASE(CT)                                                                                                       \
    case CT: hipLaunchKernelGGL(occ_gather_kernel<CT>, grid, block, 0, s, d_rgb, d_sigma, slot, M, (uint32_t)C, d_rgb_live, d_sigma_live); \
      break;
    PXO_GATHER_CASE(3) PXO_GATHER_CASE(12) PXO_GATHER_CASE(27) PXO_GATHER_CASE(48) PXO_GATHER_CASE(75)
#undef PXO_GATHER_CASE
    default: hipLaunchKernelGGL(occ_gather_kernel<0>, grid, block, 0, s, d_rgb, d_sigma, slot, M, (uint32_t)C, d_rgb_live, d_sigma_live);
  }
  return check_launch("occ_gather");
}

int launch_occ_tail_slots(int32_t* slot, int64_t n, int64_t first, hipStream_t s) {
  hipLaunchKernelGGL(occ_tail_slots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slot, n, (int32_t)first);
  return check_launch("occ_tail_slots");
}

}  // namespace pxo

using namespace pxo;

extern "C" {

int pxo_occ_pack(const float* sigma, int reso, float sigma_thresh, int dilate, uint32_t* bits, void* stream) {
  PXO_REQUIRE(reso >= 1 && reso <= PXO_OCC_MAX_RESO, "pxo_occ_pack: reso %d outside [1,%d]", reso, PXO_OCC_MAX_RESO);
  PXO_REQUIRE(dilate == 0 || dilate == 1, "pxo_occ_pack: dilate %d is not 0 / 1", dilate);
  PXO_REQUIRE(sigma && bits, "pxo_occ_pack: null pointer");
  const uint32_t n = (uint32_t)reso * (uint32_t)reso * (uint32_t)reso;      // <= 2^30
  const uint32_t nwords = (n + 31u) / 32u;
  hipLaunchKernelGGL(occ_pack_kernel, dim3((nwords + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, sigma, reso, n, sigma_thresh,
                     dilate, bits, nwords);
  return check_launch("occ_pack");
}

int pxo_occ_cull_workspace_bytes(int64_t M, size_t* bytes) {
  PXO_REQUIRE(bytes && M >= 0 && M < ((int64_t)1 << 31), "pxo_occ_cull_workspace_bytes: bad arguments (M = %lld must be in [0, 2^31))",
              (long long)M);
  *bytes = occ_cull_workspace_bytes(M);
  return PXO_OK;
}

int pxo_occ_cull(const PxoOccGrid* occ, const float* pts, int64_t M, float* pts_live, int32_t* slot, int64_t* n_live_dev, void* ws,
                 size_t ws_bytes, void* stream) {
  if (int rc = occ_validate(occ, "pxo_occ_cull")) return rc;
  PXO_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "pxo_occ_cull: %lld points outside [0, 2^31) (slot is int32)", (long long)M);
  PXO_REQUIRE(n_live_dev, "pxo_occ_cull: null n_live_dev");
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {                                       // no point: the count is still written
    if (hipMemsetAsync(n_live_dev, 0, sizeof(int64_t), s) != hipSuccess) {
      set_error("pxo_occ_cull: %s", hipGetErrorString(hipGetLastError()));
      return PXO_ERR_HIP;
    }
    return PXO_OK;
  }
  PXO_REQUIRE(pts && pts_live && slot && ws, "pxo_occ_cull: null pointer");
  const size_t need = occ_cull_workspace_bytes(M);
  if (ws_bytes < need) {
    set_error("pxo_occ_cull: workspace %zu < %zu", ws_bytes, need);
    return PXO_ERR_WORKSPACE;
  }
  return launch_occ_cull(*occ, pts, M, pts_live, slot, n_live_dev, ws, s);
}

int pxo_occ_expand(const float* raw_rgb_live, const float* raw_sigma_live, const int32_t* slot, int64_t M, int C, float* raw_rgb,
                   float* raw_sigma, void* stream) {
  PXO_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "pxo_occ_expand: %lld rows outside [0, 2^31)", (long long)M);
  PXO_REQUIRE(C >= 1 && C <= PXO_OCC_MAX_CHANNELS, "pxo_occ_expand: C = %d outside [1,%d]", C, PXO_OCC_MAX_CHANNELS);
  if (M == 0) return PXO_OK;
  // the compact arrays may be NULL when no row is live (every slot is -1: they are never read)
  PXO_REQUIRE(slot && raw_rgb && raw_sigma, "pxo_occ_expand: null pointer");
  return launch_occ_expand(raw_rgb_live, raw_sigma_live, slot, M, C, raw_rgb, raw_sigma, (hipStream_t)stream);
}

int pxo_occ_gather(const float* d_raw_rgb, const float* d_raw_sigma, const int32_t* slot, int64_t M, int C, float* d_rgb_live,
                   float* d_sigma_live, void* stream) {
  PXO_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "pxo_occ_gather: %lld rows outside [0, 2^31)", (long long)M);
  PXO_REQUIRE(C >= 1 && C <= PXO_OCC_MAX_CHANNELS, "pxo_occ_gather: C = %d outside [1,%d]", C, PXO_OCC_MAX_CHANNELS);
  if (M == 0) return PXO_OK;
  PXO_REQUIRE(d_raw_rgb && d_raw_sigma && slot && d_rgb_live && d_sigma_live, "pxo_occ_gather: null pointer");
  return launch_occ_gather(d_raw_rgb, d_raw_sigma, slot, M, C, d_rgb_live, d_sigma_live, (hipStream_t)stream);
}

}  // extern "C"
