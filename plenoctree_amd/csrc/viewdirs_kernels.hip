// View-conditioned ("vanilla") NeRF head and its fused projection onto spherical harmonics for gfx950 (MI355X).
//
// Replaces, for extraction only, MLP.forward with a condition (octree/nerf/model_utils.py:126-157), NerfModel.eval_points_raw
// with viewdirs (octree/nerf/models.py:211-252), project_nerf_to_sh (octree/extraction.py:217-241) and ProjectFunctionNeRF
// (octree/nerf/sh_proj.py:278-306), with net_depth_condition = 1, net_width_condition = 128, deg_view = 4.
//
//   x7      = trunk(posenc(p, 0, 10))                 the fused float32 MFMA trunk of mlp_kernels.hip (saved-tensor form: x7 is
//                                                     the last of its saved activations)
//   sigma   = Dense_8(x7)                             the same launch (its head holds Dense_8 and an empty colour block)
//   A[p]    = Dense_9(x7) . W10[:256]                 vd_head_kernel      [N,128], once per point
//   C[r]    = posenc(d_r, 0, 4) . W10[256:] + b10     vd_dir_kernel       [R,128], once per direction set
//   rgb     = relu(A[p] + C[r]) . W11 + b11           vd_pair_kernel      Dense_10 is linear before its ReLU, so its input splits
//   coeff[p,c,k] = 4 pi / R sum_r rgb[p,r,c] Y_k(d_r)   vd_pair_kernel    nothing of size N x R exists in memory
//
// vd_pair_kernel: ONE THREAD PER POINT.  A[p] sits in 128 registers; C[r], W11 and Y[r] are the same for every lane, so they
// are read through wave-uniform addresses (scalar loads, operands of the vector ALU straight from scalar registers); the 3K
// running sums stay in registers.  Per (point, direction) pair: 128 x (add, max, 3 fma) + 3K fma = 640 + 3K vector-ALU lane
// operations, no LDS, no cross-lane step.  The alternatives on the matrix pipe pad the 128 -> 3 contraction to 16 columns
// (mfma_f32_16x16x4: 4096 FLOP per pair) or re-associate to Y^T . relu(A + C) (2 . K . 128 = 4096 FLOP at K = 16, 6400 at
// K = 25), and both still pay the 256 add/max per pair on the vector ALU: at 157 TFLOP/s of float32 MFMA that bounds them at
// 38 G pairs/s, below the 57 G pairs/s of 688 vector operations at 39.3 T lane-operations/s.
// The sum over r runs in blocks of 8 directions (block sum, then total += block) in a fixed order that depends on r alone: a
// point's result does not depend on where it sits in the batch, and the round-off of an R-term float32 sum stays that of a
// blocked sum.
#include <cstring>

#include "pxo_common.h"
#include "pxo_sh.h"

namespace pxo {

constexpr int kVdWc = PXO_VD_WIDTH_CONDITION;   // 128
constexpr int kVdDirEnc = PXO_VD_DIR_ENC;       // 27
constexpr int kVdYStride = 25;                  // basis rows hold SH25; a lower degree reads a prefix
constexpr int64_t kVdTrunk = 493056;            // floats of Dense_0..7: the same leaves, at the same offsets, as an SH model's
// head leaves, offsets relative to the head block (Dense_8 ..) of ONE MLP's sub-arena
constexpr int64_t kW9 = 256 + 1, kB9 = kW9 + 256 * 256, kW10 = kB9 + 256, kB10 = kW10 + (256 + kVdDirEnc) * kVdWc,
                  kW11 = kB10 + kVdWc, kB11 = kW11 + kVdWc * 3, kVdHeadFloats = kB11 + 3;
static_assert(kVdTrunk + kVdHeadFloats == 595844, "view-conditioned MLP: 595,844 parameters");

__host__ __device__ inline int64_t vd_image_floats() { return fwd_image_floats(0) + kVdHeadFloats; }

// the forward image of an SH model of degree 0 keeps Dense_9 (rgb) in head columns 0..2: empty here
__global__ void vd_clear_rgb_head_kernel(float* __restrict__ img) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 256 * 3) img[fwd_layer_off(8) + packed_index(t / 3, t % 3, head_blocks(0))] = 0.f;
  if (t < 3) img[fwd_bias_off(0) + 8 * kW + t] = 0.f;
}

__global__ void vd_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// column i of posenc(d, 0, 4): [d | sin(d 2^l) | sin(d 2^l + pi/2)], xb index = l * 3 + axis (model_utils.py:161-190)
__device__ __forceinline__ float dir_enc_value(float d0, float d1, float d2, int col) {
  if (col < 3) return col == 0 ? d0 : (col == 1 ? d1 : d2);
  int idx = col - 3;
  const bool shifted = idx >= 12;
  if (shifted) idx -= 12;
  const int l = idx / 3, a = idx - 3 * l;
  float xb = (a == 0 ? d0 : (a == 1 ? d1 : d2)) * (float)(1 << l);
  if (shifted) xb = xb + 1.5707963267948966f;
  return sinf(xb);
}

constexpr int kPairThreads = 256;
constexpr int kDirBlock = 8;       // directions per block of the sum over r; C and the basis are padded to whole blocks
__host__ __device__ inline int64_t dir_blocks(int64_t R) { return (R + kDirBlock - 1) / kDirBlock; }
__host__ __device__ inline int64_t basis_index(int64_t r, int k) { return r * kVdYStride + k; }

// C[r][j] = sum_i enc_i(d_r) W10[256 + i][j] + b10[j]; Y[r][0..25) = SH basis of d_r (Y may be NULL).
// One block per direction; rows R .. gridDim.x - 1 are the padding of the last block of 8: C = 0, basis = 0 (their pairs add
// exact zeros to the projection).
__global__ __launch_bounds__(kVdWc) void vd_dir_kernel(const float* __restrict__ dirs, const float* __restrict__ head, int64_t R,
                                                       float* __restrict__ C, float* __restrict__ Y) {
  const int64_t r = blockIdx.x;
  const int j = threadIdx.x;
  if (r >= R) {
    C[r * kVdWc + j] = 0.f;
    if (Y && j < kVdYStride) Y[basis_index(r, j)] = 0.f;
    return;
  }
  const float d0 = dirs[r * 3], d1 = dirs[r * 3 + 1], d2 = dirs[r * 3 + 2];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < kVdDirEnc; ++i) acc = fmaf(dir_enc_value(d0, d1, d2, i), head[kW10 + (int64_t)(256 + i) * kVdWc + j], acc);
  C[r * kVdWc + j] = acc + head[kB10 + j];
  if (Y && j == 0) {
    float y[25];
    sh_basis<4>(d0, d1, d2, y);
#pragma unroll
    for (int k = 0; k < 25; ++k) Y[basis_index(r, k)] = y[k];
  }
}

// A = (x7 . W9 + b9) . W10[:256] (sigma = Dense_8(x7) comes from the trunk launch's own head, like pxo_grid_sigma's).  16 points
// per workgroup; every dot product runs as four interleaved chains (k mod 4) that are added pairwise at the end.  The three
// steps are __device__ functions shared by vd_head_kernel (A to memory: the projection and the per-point form) and
// vd_ray_head_kernel (A stays in LDS: ray rendering), so that both produce the same bits.
constexpr int kHeadPts = 16;
constexpr int kHeadLd = 260;
// x7 rows [row0, row0 + 16) -> xs (rows past N: zeros)
__device__ __forceinline__ void head_load_x7(const float* __restrict__ x7, int64_t row0, int64_t N, float* __restrict__ xs, int t) {
  for (int i = t; i < kHeadPts * 64; i += 256) {
    const int p = i >> 6, q = i & 63;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + p < N) v = *reinterpret_cast<const float4*>(x7 + (row0 + p) * kW + 4 * q);
    *reinterpret_cast<float4*>(&xs[p * kHeadLd + 4 * q]) = v;
  }
}
// bottleneck (Dense_9) column t of the 16 points: xs -> bs
__device__ __forceinline__ void head_bottleneck(const float* __restrict__ xs, float* __restrict__ bs, const float* __restrict__ head,
                                                int t) {
  float acc[kHeadPts][4];
#pragma unroll
  for (int p = 0; p < kHeadPts; ++p) acc[p][0] = acc[p][1] = acc[p][2] = acc[p][3] = 0.f;
  for (int k = 0; k < kW; k += 4) {
    const float w0 = head[kW9 + (int64_t)(k + 0) * kW + t], w1 = head[kW9 + (int64_t)(k + 1) * kW + t],
                w2 = head[kW9 + (int64_t)(k + 2) * kW + t], w3 = head[kW9 + (int64_t)(k + 3) * kW + t];
#pragma unroll
    for (int p = 0; p < kHeadPts; ++p) {
      const float4 x = *reinterpret_cast<const float4*>(&xs[p * kHeadLd + k]);
      acc[p][0] = fmaf(x.x, w0, acc[p][0]);
      acc[p][1] = fmaf(x.y, w1, acc[p][1]);
      acc[p][2] = fmaf(x.z, w2, acc[p][2]);
      acc[p][3] = fmaf(x.w, w3, acc[p][3]);
    }
  }
  const float b = head[kB9 + t];
#pragma unroll
  for (int p = 0; p < kHeadPts; ++p) bs[p * kHeadLd + t] = ((acc[p][0] + acc[p][1]) + (acc[p][2] + acc[p][3])) + b;
}
// A column j = t & 127 of the 8 points (t >> 7) * 8 .. + 7: bs -> a
__device__ __forceinline__ void head_condition(const float* __restrict__ bs, const float* __restrict__ head, int t, float (&a)[8]) {
  const int j = t & (kVdWc - 1), ph = t >> 7;
  float acc[8][4];
#pragma unroll
  for (int p = 0; p < 8; ++p) acc[p][0] = acc[p][1] = acc[p][2] = acc[p][3] = 0.f;
  for (int k = 0; k < kW; k += 4) {
    const float w0 = head[kW10 + (int64_t)(k + 0) * kVdWc + j], w1 = head[kW10 + (int64_t)(k + 1) * kVdWc + j],
                w2 = head[kW10 + (int64_t)(k + 2) * kVdWc + j], w3 = head[kW10 + (int64_t)(k + 3) * kVdWc + j];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const float4 x = *reinterpret_cast<const float4*>(&bs[(ph * 8 + p) * kHeadLd + k]);
      acc[p][0] = fmaf(x.x, w0, acc[p][0]);
      acc[p][1] = fmaf(x.y, w1, acc[p][1]);
      acc[p][2] = fmaf(x.z, w2, acc[p][2]);
      acc[p][3] = fmaf(x.w, w3, acc[p][3]);
    }
  }
#pragma unroll
  for (int p = 0; p < 8; ++p) a[p] = (acc[p][0] + acc[p][1]) + (acc[p][2] + acc[p][3]);
}

__global__ __launch_bounds__(256) void vd_head_kernel(const float* __restrict__ x7, const float* __restrict__ head, int64_t N,
                                                      float* __restrict__ A) {
  __shared__ __attribute__((aligned(16))) float xs[kHeadPts * kHeadLd];
  __shared__ __attribute__((aligned(16))) float bs[kHeadPts * kHeadLd];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kHeadPts;
  head_load_x7(x7, row0, N, xs, t);
  __syncthreads();
  head_bottleneck(xs, bs, head, t);
  __syncthreads();
  float a[8];
  head_condition(bs, head, t, a);
  const int j = t & (kVdWc - 1), ph = t >> 7;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int64_t row = row0 + ph * 8 + p;
    if (row < N) A[row * kVdWc + j] = a[p];
  }
}

// channels [c0, c0 + NC) of one row's raw colour: relu(a + c) . W11 + b11, two chains (j parity) per channel
template <int NC>
__device__ __forceinline__ void row_rgb(const float* __restrict__ a, const float* __restrict__ c, const float* __restrict__ head,
                                        int c0, float* __restrict__ out) {
  float s0[NC], s1[NC];
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) s0[ch] = s1[ch] = 0.f;
  for (int j = 0; j < kVdWc; j += 2) {
    const float h0 = fmaxf(a[j] + c[j], 0.f), h1 = fmaxf(a[j + 1] + c[j + 1], 0.f);
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      s0[ch] = fmaf(h0, head[kW11 + j * 3 + c0 + ch], s0[ch]);
      s1[ch] = fmaf(h1, head[kW11 + (j + 1) * 3 + c0 + ch], s1[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) out[ch] = (s0[ch] + s1[ch]) + head[kB11 + c0 + ch];
}

// Ray rendering: raw_rgb[row] = relu(A[row] + C[row / S]) . W11 + b11 for 16 consecutive sample rows, A = Dense_9(x7) . W10[:256]
// computed in LDS by the functions above and never written to memory (the vd_head_kernel + vd_point_kernel pair moves 1 KB per
// sample through it, and needs C per sample instead of per ray).  C [rays,128]: vd_dir_kernel on the block's view directions.
// The ray of a row is looked up per row: a group of 16 straddles two rays whenever S is not a multiple of 16.
__global__ __launch_bounds__(256) void vd_ray_head_kernel(const float* __restrict__ x7, const float* __restrict__ head,
                                                          const float* __restrict__ C, int64_t M, int S,
                                                          float* __restrict__ raw_rgb) {
  __shared__ __attribute__((aligned(16))) float xs[kHeadPts * kHeadLd];
  __shared__ __attribute__((aligned(16))) float bs[kHeadPts * kHeadLd];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kHeadPts;
  head_load_x7(x7, row0, M, xs, t);
  __syncthreads();
  head_bottleneck(xs, bs, head, t);
  __syncthreads();
  float a[8];
  head_condition(bs, head, t, a);
  const int j = t & (kVdWc - 1), ph = t >> 7;
#pragma unroll
  for (int p = 0; p < 8; ++p) xs[(ph * 8 + p) * kHeadLd + j] = a[p];      // xs was last read before the second barrier
  for (int i = t; i < kHeadPts * kVdWc; i += 256) {                        // C of each row's ray -> columns 128.. of xs
    const int p = i >> 7, jj = i & (kVdWc - 1);
    const int64_t row = row0 + p < M ? row0 + p : M - 1;
    xs[p * kHeadLd + kVdWc + jj] = C[(row / S) * kVdWc + jj];
  }
  __syncthreads();
  if (t < kHeadPts * 3) {
    const int p = t / 3, ch = t - 3 * p;
    float v;
    row_rgb<1>(&xs[p * kHeadLd], &xs[p * kHeadLd + kVdWc], head, ch, &v);
    if (row0 + p < M) raw_rgb[(row0 + p) * 3 + ch] = v;
  }
}

// rgb of one (point, direction) pair: relu(a + c) . W11 + b11, two chains (j parity).  c, w and b are wave-uniform.
__device__ __forceinline__ void pair_rgb(const float (&a)[kVdWc], const float* __restrict__ c, const float* __restrict__ w,
                                         const float* __restrict__ b, float (&rgb)[3]) {
  float s0[3] = {0.f, 0.f, 0.f}, s1[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kVdWc; j += 2) {
    const float h0 = fmaxf(a[j] + c[j], 0.f), h1 = fmaxf(a[j + 1] + c[j + 1], 0.f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      s0[ch] = fmaf(h0, w[j * 3 + ch], s0[ch]);
      s1[ch] = fmaf(h1, w[(j + 1) * 3 + ch], s1[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = (s0[ch] + s1[ch]) + b[ch];
}

// PROJECT: out = coeffs [N, 3K] (channel-major); else out = raw_rgb [N, R, 3] (the materialising parity hook).
// w_step is 0: Dense_11's 384 weights are addressed as head + r * w_step so that their (scalar) loads stay inside the loop over
// r -- hoisted out of it they would not fit the scalar register file.
template <int DEG, bool PROJECT>
__global__ __launch_bounds__(kPairThreads) void vd_pair_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                              const float* __restrict__ Y, const float* __restrict__ head,
                                                              int64_t N, int R, int w_step, float weight,
                                                              float* __restrict__ out) {
  constexpr int K = (DEG + 1) * (DEG + 1);
  constexpr int NT = PROJECT ? 3 * K : 1;
  const int64_t p = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  const int64_t pc = p < N ? p : N - 1;        // lanes past the end redo the last point and store nothing
  float a[kVdWc];
#pragma unroll
  for (int j = 0; j < kVdWc; j += 4) {
    const float4 v = *reinterpret_cast<const float4*>(A + pc * kVdWc + j);
    a[j] = v.x; a[j + 1] = v.y; a[j + 2] = v.z; a[j + 3] = v.w;
  }
  float tot[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tot[i] = 0.f;
  const int nblk = (int)dir_blocks(R);
  for (int b = 0; b < nblk; ++b) {
    float blk[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) blk[i] = 0.f;
#pragma unroll 1
    for (int d = 0; d < kDirBlock; ++d) {
      const int r = b * kDirBlock + d;
      const float* __restrict__ hw = head + (int64_t)r * w_step;
      float rgb[3];
      pair_rgb(a, C + (int64_t)r * kVdWc, hw + kW11, hw + kB11, rgb);
      if constexpr (PROJECT) {
        const float* __restrict__ y = Y + (int64_t)r * kVdYStride;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float yk = y[k];
          blk[k] = fmaf(rgb[0], yk, blk[k]);
          blk[K + k] = fmaf(rgb[1], yk, blk[K + k]);
          blk[2 * K + k] = fmaf(rgb[2], yk, blk[2 * K + k]);
        }
      } else if (p < N && r < R) {
        float* o = out + (p * R + r) * 3;
        o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
      }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) tot[i] += blk[i];
  }
  if constexpr (PROJECT) {
    if (p < N) {
#pragma unroll
      for (int i = 0; i < 3 * K; ++i) out[p * (3 * K) + i] = tot[i] * weight;
    }
  }
}

// one direction per point: Cn [N,128] holds C of point p's own direction
__global__ __launch_bounds__(kPairThreads) void vd_point_kernel(const float* __restrict__ A, const float* __restrict__ Cn,
                                                               const float* __restrict__ head, int64_t N,
                                                               float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  if (p >= N) return;
  row_rgb<3>(A + p * kVdWc, Cn + p * kVdWc, head, 0, out + p * 3);
}

namespace {

struct VdCarver {      // bump allocator over the caller's workspace; with base == nullptr it only measures
  char* base;
  size_t off = 0;
  explicit VdCarver(void* b) : base(reinterpret_cast<char*>(b)) {}
  template <typename T>
  T* take(int64_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (size_t)count * sizeof(T);
    return p;
  }
};

struct VdWs {
  float *acts, *enc, *A, *C, *Y;
  uint32_t* mask;
  size_t total;
};

// n_c rows of C (R for a shared direction set, N for one direction per point); n_y rows of the basis (0: none)
void vd_carve(void* ws, int64_t N, int64_t n_c, int64_t n_y, VdWs& w) {
  VdCarver c(ws);
  const int64_t n = N > 0 ? N : 1;
  w.acts = c.take<float>(n * kW * kDepth);
  w.enc = c.take<float>(n * kEncPad);
  w.mask = c.take<uint32_t>(mask_words(n));
  w.A = c.take<float>(n * kVdWc);
  w.C = c.take<float>((dir_blocks(n_c) + 1) * kDirBlock * kVdWc);
  w.Y = c.take<float>((dir_blocks(n_y) + 1) * kDirBlock * kVdYStride);
  w.total = (c.off + 255) & ~(size_t)255;
}

PxoCfg trunk_cfg() {       // the SH model of degree 0 whose forward image carries the trunk and Dense_8
  PxoCfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.num_coarse_samples = 64;
  cfg.num_fine_samples = 128;
  cfg.sh_deg = 0;
  cfg.max_deg_point = 10;
  cfg.mlp_precision = PXO_MLP_F32;
  return cfg;
}

int vd_precision(int mlp_precision, const char* what) {
  if (mlp_precision == PXO_MLP_F32) return PXO_OK;
  if (mlp_precision == PXO_MLP_BF16X3 || mlp_precision == PXO_MLP_BF16X6) {
    set_error("%s: the view-conditioned head is built in float32 only (mlp_precision %d)", what, mlp_precision);
    return PXO_ERR_UNSUPPORTED;
  }
  set_error("%s: mlp_precision %d unknown", what, mlp_precision);
  return PXO_ERR_ARG;
}

// trunk + head for N points: fills sigma and w.A
int vd_points(const float* packed, const float* points, int64_t N, float* raw_sigma, VdWs& w, hipStream_t s) {
  const PxoCfg cfg = trunk_cfg();
  int rc = launch_mlp_fwd(&cfg, packed, points, N, nullptr, raw_sigma, w.acts, w.enc, w.mask, s);
  if (rc != PXO_OK) return rc;
  const float* x7 = w.acts + (int64_t)(kDepth - 1) * N * kW;
  const float* head = packed + fwd_image_floats(0);
  hipLaunchKernelGGL(vd_head_kernel, dim3((unsigned)((N + kHeadPts - 1) / kHeadPts)), dim3(256), 0, s, x7, head, N, w.A);
  return check_launch("vd_head");
}

template <bool PROJECT>
int launch_pair(int sh_deg, const float* A, const float* C, const float* Y, const float* head, int64_t N, int R, float weight,
                float* out, hipStream_t s) {
  const dim3 grid((unsigned)((N + kPairThreads - 1) / kPairThreads)), block(kPairThreads);
  switch (sh_deg) {
    case 0: hipLaunchKernelGGL((vd_pair_kernel<0, PROJECT>), grid, block, 0, s, A, C, Y, head, N, R, 0, weight, out); break;
    case 1: hipLaunchKernelGGL((vd_pair_kernel<1, PROJECT>), grid, block, 0, s, A, C, Y, head, N, R, 0, weight, out); break;
    case 2: hipLaunchKernelGGL((vd_pair_kernel<2, PROJECT>), grid, block, 0, s, A, C, Y, head, N, R, 0, weight, out); break;
    case 3: hipLaunchKernelGGL((vd_pair_kernel<3, PROJECT>), grid, block, 0, s, A, C, Y, head, N, R, 0, weight, out); break;
    default: hipLaunchKernelGGL((vd_pair_kernel<4, PROJECT>), grid, block, 0, s, A, C, Y, head, N, R, 0, weight, out); break;
  }
  return check_launch(PROJECT ? "vd_project" : "vd_eval_cross");
}

constexpr int64_t kVdMaxRows = (int64_t)1 << 30;    // keeps every grid dimension and every index product in range

// ---- ray rendering ------------------------------------------------------------------------------------------------------------
// Workspace of pxo_vd_render_fwd: the buffers of ONE block of `rb` rays at S = Nc + Nf samples (the coarse level uses a prefix of
// them: its points, raw values and saved tensors are dead once its weights exist), and the draws of the whole batch.
struct VdRenderWs {
  float *acts, *enc, *z_c, *w_c, *z_f, *pts, *raw_sigma, *raw_rgb, *C, *t_rand, *u;
  uint32_t* mask;
  int64_t rb;
  size_t total;
};

void vd_render_carve(const PxoCfg* cfg, int64_t B, int block, void* ws, VdRenderWs& w) {
  VdCarver c(ws);
  const int Nc = cfg->num_coarse_samples, Nf = cfg->num_fine_samples, S = Nc + Nf;
  w.rb = B < block ? (B > 0 ? B : 1) : block;
  const int64_t n = w.rb * S;
  w.acts = c.take<float>(n * kW * kDepth);
  w.enc = c.take<float>(n * kEncPad);
  w.mask = c.take<uint32_t>(mask_words(n));
  w.z_c = c.take<float>(w.rb * Nc);
  w.w_c = c.take<float>(w.rb * Nc);
  w.z_f = c.take<float>(n);
  w.pts = c.take<float>(n * 3);
  w.raw_sigma = c.take<float>(n);
  w.raw_rgb = c.take<float>(n * 3);
  w.C = c.take<float>((dir_blocks(w.rb) + 1) * kDirBlock * kVdWc);
  w.t_rand = c.take<float>(B * Nc);
  w.u = c.take<float>(B * (Nf > 0 ? Nf : 1));
  w.total = (c.off + 255) & ~(size_t)255;
}

// one level of one block: trunk (raw sigma, x7), the direction term once per ray, the fused head (raw colour)
int vd_render_level(const float* packed, int64_t nb, int S, const float* viewdirs, VdRenderWs& w, hipStream_t s) {
  const PxoCfg tcfg = trunk_cfg();
  const int64_t M = nb * S;
  int rc = launch_mlp_fwd(&tcfg, packed, w.pts, M, nullptr, w.raw_sigma, w.acts, w.enc, w.mask, s);
  if (rc != PXO_OK) return rc;
  const float* x7 = w.acts + (int64_t)(kDepth - 1) * M * kW;
  const float* head = packed + fwd_image_floats(0);
  hipLaunchKernelGGL(vd_dir_kernel, dim3((unsigned)(dir_blocks(nb) * kDirBlock)), dim3(kVdWc), 0, s, viewdirs, head, nb, w.C,
                     (float*)nullptr);
  rc = check_launch("vd_dir");
  if (rc != PXO_OK) return rc;
  hipLaunchKernelGGL(vd_ray_head_kernel, dim3((unsigned)((M + kHeadPts - 1) / kHeadPts)), dim3(256), 0, s, x7, head, w.C, M, S,
                     w.raw_rgb);
  return check_launch("vd_ray_head");
}

// the cfg checks of the SH entry points, without sh_deg (this model has none: the reference's rendering presets say -1)
int vd_render_cfg(const PxoCfg* cfg, const char* what) {
  PXO_REQUIRE(cfg != nullptr, "%s: cfg is NULL", what);
  PxoCfg c = *cfg;
  c.sh_deg = 0;
  const int rc = validate_cfg(&c);
  return rc != PXO_OK ? rc : vd_precision(cfg->mlp_precision, what);
}

}  // namespace
}  // namespace pxo

using namespace pxo;

extern "C" {

int pxo_vd_param_layout(PxoLeaf* leaves, int64_t* floats_per_mlp) {
  if (leaves) {
    int64_t off = 0;
    for (int l = 0; l < 12; ++l) {
      const int in = l < 8 ? layer_in(l) : (l < 10 ? kW : (l == 10 ? kW + kVdDirEnc : kVdWc));
      const int out = l < 8 ? kW : (l == 8 ? 1 : (l == 9 ? kW : (l == 10 ? kVdWc : 3)));
      leaves[2 * l] = PxoLeaf{l, 0, off, in, out};
      off += (int64_t)in * out;
      leaves[2 * l + 1] = PxoLeaf{l, 1, off, out, 1};
      off += out;
    }
  }
  if (floats_per_mlp) *floats_per_mlp = kVdTrunk + kVdHeadFloats;
  return PXO_OK;
}

int pxo_vd_packed_floats(int64_t* floats) {
  PXO_REQUIRE(floats != nullptr, "pxo_vd_packed_floats: NULL pointer");
  *floats = vd_image_floats();
  return PXO_OK;
}

int pxo_vd_pack_weights(const float* mlp_params, float* packed, void* stream) {
  PXO_REQUIRE(mlp_params && packed, "pxo_vd_pack_weights: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  // Dense_0..8 sit where an SH model of degree 0 keeps them, so its packing kernel writes the trunk and the sigma column;
  // what it read as that model's rgb head (the first floats of Dense_9) is cleared again
  const PxoCfg cfg = trunk_cfg();
  int rc = launch_pack(&cfg, mlp_params, packed, nullptr, s);
  if (rc != PXO_OK) return rc;
  hipLaunchKernelGGL(vd_clear_rgb_head_kernel, dim3(3), dim3(256), 0, s, packed);
  hipLaunchKernelGGL(vd_copy_kernel, dim3(128), dim3(256), 0, s, mlp_params + kVdTrunk, packed + fwd_image_floats(0), kVdHeadFloats);
  return check_launch("vd_pack_weights");
}

int pxo_vd_eval_workspace_bytes(int64_t N, int64_t R, int cross_broadcast, size_t* bytes) {
  PXO_REQUIRE(bytes && N >= 0 && N <= kVdMaxRows && R >= 0 && R <= kVdMaxRows, "pxo_vd_eval_workspace_bytes: bad arguments");
  VdWs w;
  vd_carve(nullptr, N, cross_broadcast ? R : N, 0, w);
  *bytes = w.total;
  return PXO_OK;
}

int pxo_vd_eval_points_raw(int mlp_precision, const float* packed, const float* points, int64_t N, const float* viewdirs,
                           int64_t R, int cross_broadcast, float* raw_rgb, float* raw_sigma, void* ws, size_t ws_bytes,
                           void* stream) {
  int rc = vd_precision(mlp_precision, "pxo_vd_eval_points_raw");
  if (rc != PXO_OK) return rc;
  if (N == 0) return PXO_OK;
  PXO_REQUIRE(N > 0 && N <= kVdMaxRows && packed && points && raw_sigma && ws, "pxo_vd_eval_points_raw: bad arguments");
  PXO_REQUIRE(raw_rgb == nullptr || viewdirs != nullptr, "pxo_vd_eval_points_raw: raw_rgb needs viewdirs");
  const int64_t n_c = raw_rgb ? (cross_broadcast ? R : N) : 0;
  if (raw_rgb) {
    PXO_REQUIRE(cross_broadcast ? (R >= 0 && R <= kVdMaxRows && N * R <= ((int64_t)1 << 40)) : R == N,
                "pxo_vd_eval_points_raw: %lld directions for %lld points (cross_broadcast %d)", (long long)R, (long long)N,
                cross_broadcast);
  }
  VdWs w;
  vd_carve(ws, N, n_c, 0, w);
  if (ws_bytes < w.total) { set_error("pxo_vd_eval_points_raw: workspace %zu < %zu", ws_bytes, w.total); return PXO_ERR_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  rc = vd_points(packed, points, N, raw_sigma, w, s);
  if (rc != PXO_OK || !raw_rgb || n_c == 0) return rc;
  const float* head = packed + fwd_image_floats(0);
  hipLaunchKernelGGL(vd_dir_kernel, dim3((unsigned)(dir_blocks(n_c) * kDirBlock)), dim3(kVdWc), 0, s, viewdirs, head, n_c, w.C,
                     (float*)nullptr);
  rc = check_launch("vd_dir");
  if (rc != PXO_OK) return rc;
  if (cross_broadcast) return launch_pair<false>(0, w.A, w.C, nullptr, head, N, (int)R, 0.f, raw_rgb, s);
  hipLaunchKernelGGL(vd_point_kernel, dim3((unsigned)((N + kPairThreads - 1) / kPairThreads)), dim3(kPairThreads), 0, s, w.A, w.C,
                     head, N, raw_rgb);
  return check_launch("vd_eval_points");
}

int pxo_vd_project_workspace_bytes(int64_t N, int64_t R, size_t* bytes) {
  PXO_REQUIRE(bytes && N >= 0 && N <= kVdMaxRows && R >= 1 && R <= kVdMaxRows, "pxo_vd_project_workspace_bytes: bad arguments");
  VdWs w;
  vd_carve(nullptr, N, R, R, w);
  *bytes = w.total;
  return PXO_OK;
}

int pxo_vd_project_sh(int mlp_precision, const float* packed, const float* points, int64_t N, const float* dirs, int64_t R,
                      int sh_deg, float* coeffs, float* raw_sigma, void* ws, size_t ws_bytes, void* stream) {
  int rc = vd_precision(mlp_precision, "pxo_vd_project_sh");
  if (rc != PXO_OK) return rc;
  PXO_REQUIRE(sh_deg >= 0 && sh_deg <= 4, "pxo_vd_project_sh: sh_deg %d not in [0,4] (octree/nerf/sh_proj.py:24)", sh_deg);
  PXO_REQUIRE(R >= 1 && R <= kVdMaxRows, "pxo_vd_project_sh: %lld projection samples", (long long)R);
  if (N == 0) return PXO_OK;
  PXO_REQUIRE(N > 0 && N <= kVdMaxRows && packed && points && dirs && coeffs && raw_sigma && ws, "pxo_vd_project_sh: bad arguments");
  VdWs w;
  vd_carve(ws, N, R, R, w);
  if (ws_bytes < w.total) { set_error("pxo_vd_project_sh: workspace %zu < %zu", ws_bytes, w.total); return PXO_ERR_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  rc = vd_points(packed, points, N, raw_sigma, w, s);
  if (rc != PXO_OK) return rc;
  const float* head = packed + fwd_image_floats(0);
  hipLaunchKernelGGL(vd_dir_kernel, dim3((unsigned)(dir_blocks(R) * kDirBlock)), dim3(kVdWc), 0, s, dirs, head, R, w.C, w.Y);
  rc = check_launch("vd_dir");
  if (rc != PXO_OK) return rc;
  const float weight = (float)(4.0 * 3.14159265358979323846 / (double)R);
  return launch_pair<true>(sh_deg, w.A, w.C, w.Y, head, N, (int)R, weight, coeffs, s);
}

int pxo_vd_render_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  int rc = vd_render_cfg(cfg, "pxo_vd_render_workspace_bytes");
  if (rc != PXO_OK) return rc;
  PXO_REQUIRE(bytes && B >= 0 && B <= kVdMaxRows, "pxo_vd_render_workspace_bytes: bad arguments");
  VdRenderWs w;
  vd_render_carve(cfg, B, tuning_snapshot().vd_ray_block, nullptr, w);
  *bytes = w.total;
  return PXO_OK;
}

int pxo_vd_render_fwd(const PxoCfg* cfg, const float* packed0, const float* packed1, const float* origins,
                      const float* directions, const float* viewdirs, int64_t B, int randomized, const float* t_rand,
                      const float* u, uint64_t seed, float* rgb_c, float* disp_c, float* acc_c, float* rgb_f, float* disp_f,
                      float* acc_f, void* ws, size_t ws_bytes, void* stream) {
  int rc = vd_render_cfg(cfg, "pxo_vd_render_fwd");
  if (rc != PXO_OK) return rc;
  if (B == 0) return PXO_OK;                   // an empty batch has no buffers to check
  PXO_REQUIRE(B > 0 && B <= kVdMaxRows && packed0 && origins && directions && viewdirs && rgb_c && disp_c && acc_c && ws,
              "pxo_vd_render_fwd: bad arguments");
  const int Nc = cfg->num_coarse_samples, Nf = cfg->num_fine_samples, S = Nc + Nf;
  if (Nf > 0) PXO_REQUIRE(packed1 && rgb_f && disp_f && acc_f, "pxo_vd_render_fwd: fine outputs/weights missing");
  VdRenderWs w;
  vd_render_carve(cfg, B, tuning_snapshot().vd_ray_block, ws, w);
  if (ws_bytes < w.total) { set_error("pxo_vd_render_fwd: workspace %zu < %zu", ws_bytes, w.total); return PXO_ERR_WORKSPACE; }
  hipStream_t s = (hipStream_t)stream;
  // the draws of the whole batch (jax.random.uniform call sites model_utils.py:135,262), the streams of pxo_render_fwd
  UniformJob jobs[2];
  int nj = 0;
  if (randomized && !t_rand) { jobs[nj++] = UniformJob{0, B * Nc, 0.f, 1.f, w.t_rand}; t_rand = w.t_rand; }
  if (randomized && Nf > 0 && !u) { jobs[nj++] = UniformJob{1, B * Nf, 0.f, 1.f, w.u}; u = w.u; }
  if (!randomized) { t_rand = nullptr; u = nullptr; }
  rc = launch_uniform_jobs(seed, jobs, nj, s);
  if (rc != PXO_OK) return rc;
  const bool noisy = randomized != 0 && cfg->noise_std > 0.f;     // (noise_std is not None) and randomized, model_utils.py:329
  for (int64_t r0 = 0; r0 < B; r0 += w.rb) {
    const int64_t nb = B - r0 < w.rb ? B - r0 : w.rb;
    const float *o = origins + r0 * 3, *d = directions + r0 * 3, *v = viewdirs + r0 * 3;
    rc = launch_sample_along_rays(o, d, nb, Nc, cfg->near_, cfg->far_, cfg->lindisp, t_rand ? t_rand + r0 * Nc : nullptr, w.z_c,
                                  w.pts, s);
    if (rc != PXO_OK) return rc;
    rc = vd_render_level(packed0, nb, Nc, v, w, s);
    if (rc != PXO_OK) return rc;
    if (noisy) {                                                   // models.py:258-264
      rc = launch_add_noise(w.raw_sigma, nb * Nc, cfg->noise_std, nullptr, seed, 3, s, r0 * Nc);
      if (rc != PXO_OK) return rc;
    }
    rc = launch_vd_composite_fwd(cfg->white_bkgd, w.raw_rgb, w.raw_sigma, w.z_c, d, nb, Nc, rgb_c + r0 * 3, disp_c + r0,
                                 acc_c + r0, Nf > 0 ? w.w_c : nullptr, s);
    if (rc != PXO_OK) return rc;
    if (Nf == 0) continue;
    rc = launch_sample_pdf(w.z_c, w.w_c, o, d, nb, Nc, Nf, u ? u + r0 * Nf : nullptr, w.z_f, w.pts, s);
    if (rc != PXO_OK) return rc;
    rc = vd_render_level(packed1, nb, S, v, w, s);
    if (rc != PXO_OK) return rc;
    if (noisy) {                                                   // models.py:318-324
      rc = launch_add_noise(w.raw_sigma, nb * S, cfg->noise_std, nullptr, seed, 4, s, r0 * S);
      if (rc != PXO_OK) return rc;
    }
    rc = launch_vd_composite_fwd(cfg->white_bkgd, w.raw_rgb, w.raw_sigma, w.z_f, d, nb, S, rgb_f + r0 * 3, disp_f + r0,
                                 acc_f + r0, nullptr, s);
    if (rc != PXO_OK) return rc;
  }
  return PXO_OK;
}

int pxo_vd_composite_fwd(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, const float* z_vals,
                         const float* directions, int64_t B, int S, float* comp_rgb, float* disp, float* acc, float* weights,
                         void* stream) {
  PXO_REQUIRE(cfg != nullptr, "pxo_vd_composite_fwd: cfg is NULL");
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B > 0 && raw_rgb && raw_sigma && z_vals && directions && comp_rgb && disp && acc,
              "pxo_vd_composite_fwd: bad arguments");
  return launch_vd_composite_fwd(cfg->white_bkgd, raw_rgb, raw_sigma, z_vals, directions, B, S, comp_rgb, disp, acc, weights,
                                 (hipStream_t)stream);
}

}  // extern "C"
