// What the three precisions of the fused NeRF-SH MLP share (mlp_kernels.hip float32, mlp_x3_kernels.hip bf16x3,
// mlp_x6_kernels.hip bf16x6; included by those three units only): where a weight and a bias come from, the position
// encoding, the dense-grid point source, the relu-mask bit order, the LDS barrier, the tile ticket, and
// the launchers' dispatch on the head width.  The GEMM loops, LDS layouts, fragment orders and epilogues are each file's own.
#pragma once
#include <type_traits>
#include "pxo_common.h"

namespace pxo {

// ------------------------------------------------------------------------------------------
// weight and bias sources of the packed images
// ------------------------------------------------------------------------------------------
// W_l[k_in][n_out] of the reference layout with zero padding; l == 8 denotes the fused head
// (cols [0,C) = Dense_9, col C = Dense_8).
__device__ __forceinline__ float src_weight(const float* __restrict__ p, int deg, int l, int k, int n) {
  const int C = rgb_channels(deg);
  if (l < 8) {
    if (k >= layer_in(l) || n >= kW) return 0.f;
    return p[leaf_kernel_off(l, deg) + (int64_t)k * kW + n];
  }
  if (k >= kW) return 0.f;
  if (n < C) return p[leaf_kernel_off(9, deg) + (int64_t)k * C + n];
  if (n == C) return p[leaf_kernel_off(8, deg) + k];
  return 0.f;
}
// float b of the bias tail that ends every forward image: the 8 trunk biases, then the head's bias block in the fused
// head's column order, zero-padded to whole 32-column blocks
__device__ __forceinline__ float fwd_image_bias(const float* __restrict__ p, int deg, int b) {
  if (b < 8 * kW) return p[leaf_bias_off(b / kW, deg) + (b % kW)];
  const int n = b - 8 * kW, C = rgb_channels(deg);
  return n < C ? p[leaf_bias_off(9, deg) + n] : (n == C ? p[leaf_bias_off(8, deg)] : 0.f);
}

// ------------------------------------------------------------------------------------------
// positional encoding and the dense-grid point source
// ------------------------------------------------------------------------------------------
// column `col` of posenc(p, 0, 10) padded to 64: [p | sin(p*2^l) | sin(p*2^l + pi/2) | 0]
// (nerf_sh/nerf/model_utils.py:160-173, default order: xb index = l*3 + axis).
__device__ __forceinline__ float enc_value(float p0, float p1, float p2, int col) {
  if (col < 3) return col == 0 ? p0 : (col == 1 ? p1 : p2);
  if (col >= kEnc) return 0.f;
  int idx = col - 3;
  const bool shifted = idx >= 30;
  if (shifted) idx -= 30;
  const int l = idx / 3, a = idx - 3 * l;
  float xb = (a == 0 ? p0 : (a == 1 ? p1 : p2)) * (float)(1 << l);
  if (shifted) xb = xb + 1.5707963267948966f;
  return sinf(xb);
}

// dense-grid point source for octree.extraction step1 / auto_scale
// (octree/extraction.py:250-262, :290-303): n -> (ix, iy, iz), x slowest.
struct GridSpec {
  int enabled;
  int reso;
  int x0;
  float off[3];
  float scale[3];
};
// pts == nullptr selects the grid; a launch from points leaves reso / off / scale NULL or 0
inline GridSpec make_grid_spec(bool enabled, int reso, int x0, const float* off, const float* scale) {
  GridSpec g;
  g.enabled = enabled; g.reso = reso > 0 ? reso : 1; g.x0 = x0;
  for (int i = 0; i < 3; ++i) { g.off[i] = off ? off[i] : 0.f; g.scale[i] = scale ? scale[i] : 1.f; }
  return g;
}
__device__ __forceinline__ void grid_point(const GridSpec& g, int64_t n, float& px, float& py, float& pz) {
  const int r = g.reso;
  int iz = (int)(n % r);
  int64_t t = n / r;
  int iy = (int)(t % r);
  int ix = (int)(t / r) + g.x0;
  px = ((((float)ix + 0.5f) / (float)r) - g.off[0]) / g.scale[0];
  py = ((((float)iy + 0.5f) / (float)r) - g.off[1]) / g.scale[1];
  pz = ((((float)iz + 0.5f) / (float)r) - g.off[2]) / g.scale[2];
}

// ------------------------------------------------------------------------------------------
// scheduling fence, LDS barrier, relu-mask bit order
// ------------------------------------------------------------------------------------------
#define PXO_PIN() __builtin_amdgcn_sched_barrier(0)
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt: a wave would wait at every barrier
// for the acknowledgement of the activation-tile stores it has just issued (and for its prefetched weight fragments);
// nothing that crosses waves inside these kernels lives in global memory.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// relu mask, one bit per accumulator element, packed MSB-first in the order the epilogue visits the elements (float32: row
// block, column block, register; bf16x6: row block, quad, element): the forward epilogue shifts the bit "v > 0" in from the
// carry (mw = 2 mw + bit: compare + add-with-carry), the backward epilogue shifts it out again (mask_pop / mask_pop6).
__device__ __forceinline__ void mask_push(uint32_t& mw, float v) {
  asm volatile("v_cmp_lt_f32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mw) : "v"(v) : "vcc");
}

// ------------------------------------------------------------------------------------------
// tile schedules of the persistent workgroups (float32 and bf16x6, forward and backward(data))
// ------------------------------------------------------------------------------------------
//   static  (DYN = false)  workgroup b runs slots b, b + grid, b + 2 grid, ...
//   dynamic (DYN = true)   workgroup b runs slot b first and then TAKES slots from a device counter (zero at launch):
//                          slot = grid + atomicAdd(counter, 1).  The ticket for the NEXT slot is drawn by thread 0 when a
//                          tile starts (the atomic's round trip rides with the tile's first loads) and handed over
//                          through LDS when the tile ends: the schedule costs two LDS barriers per tile.
// Results do not depend on the schedule: a slot's rows, relu-mask words and bias partial are a function of the slot alone.
// Why dynamic: with one 8-wave workgroup per CU at the full register / LDS budget nothing else can be co-resident, so a
// collective's kernel on the high-priority exchange stream (dist.GradReducer) takes whole CUs when it starts at a kernel
// boundary; under the static stride the workgroups that start late on those CUs become the launch's tail, under the counter
// their share is absorbed by all the others (scripts/contention_probe.py).  Skipping mode (bwd) needs it for load balance.
struct TileTicket {
  int* next;                       // LDS word
  unsigned int* counter;           // device word, zero when the launch starts
  // thread 0 draws the ticket when the tile starts and keeps it in a register: the atomic's round trip then overlaps the
  // tile's first loads (its return is waited for with them) instead of holding thread 0's wave -- and with it the whole
  // workgroup at the tile's first barrier -- for ~1 us
  __device__ __forceinline__ int draw(int tid) const {
    return tid == 0 ? (int)gridDim.x + (int)atomicAdd(counter, 1u) : 0;
  }
  __device__ __forceinline__ int64_t take(int tid, int ticket) const {
    if (tid == 0) *next = ticket;
    lds_barrier();                 // the ticket is in LDS (and every wave is through the tile)
    const int v = __builtin_amdgcn_readfirstlane(*next);
    lds_barrier();                 // everyone has read it before thread 0 overwrites it
    return v;
  }
};
// The walk itself, for (slot = blockIdx.x; slot < n_slots;) { draw; run the slot; slot = take; }, is written out in the four
// kernels that use it: behind a function template hipcc lays out and schedules every one of them differently, the float32
// training kernels included (profiles/EXPERIMENTS.md, "one copy of what the MLP precisions share").

// ------------------------------------------------------------------------------------------
// launch dispatch
// ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, NHB>) for the number of 32-column head blocks of the configuration's SH degree
template <typename F>
static auto head_switch(int deg, F&& f) {
  switch (head_blocks(deg)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
  }
}

}  // namespace pxo
