// Shared host/device definitions for the gfx950 NeRF-SH kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/plenoctree_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace pxo {

constexpr int kW = PXO_NET_WIDTH;        // 256
constexpr int kDepth = PXO_NET_DEPTH;    // 8
constexpr int kEnc = PXO_ENC_DIM;        // 63
constexpr int kEncPad = PXO_ENC_PAD;     // 64
// Geometry of the fused MLP kernels: 128-row tiles, 8 waves (every wave owns all rows x 32 columns of a layer),
// one persistent workgroup per CU.  One weight-fragment load then feeds 16 MFMAs (scripts/ubench/gemm_geom.hip:
// 149.7 TFLOP/s for the bare loop against 138.3 for 64 x 64 per wave).
constexpr int kTM = 128;
constexpr int kMlpThreads = 512;
constexpr int kMlpWgPerCu = 1;
constexpr int kLDA = 260;                // LDS row stride (floats): 256 + one b128 access of pad
constexpr int kMlpWaves = kMlpThreads / 64;
constexpr int kMaskWords = (kTM / 32) * (8 / kMlpWaves) * 16 / 32;  // relu-mask words per thread per layer
constexpr int kMaxMlpGrid = 1024;        // upper bound on persistent workgroups
constexpr int kLiveRows = 16;            // rows per "live" flag of the zero-row skipping backward (= the wgrad chunk height)
constexpr int kMaxLiveChunks = 2048;     // live-chunk list of a SPARSE wgrad workgroup (LDS): row ranges of at most 32,768 rows

// ---- derived sizes -----------------------------------------------------------------
__host__ __device__ inline int sh_dim(int deg) { return (deg + 1) * (deg + 1); }
__host__ __device__ inline int rgb_channels(int deg) { return 3 * sh_dim(deg); }
// head width padded to 32-col MFMA blocks: cols [0,3K) = Dense_9 (rgb), col 3K = Dense_8 (sigma)
__host__ __device__ inline int head_blocks(int deg) { return (rgb_channels(deg) + 1 + 31) / 32; }

// input rows of Dense_l (l = 0..9) in the reference layout
__host__ __device__ inline int layer_in(int l) {
  return l == 0 ? kEnc : (l == 5 ? kW + kEnc : kW);
}
__host__ __device__ inline int layer_out(int l, int deg) {
  return l < 8 ? kW : (l == 8 ? 1 : rgb_channels(deg));
}
// offset (floats) of Dense_l kernel inside ONE MLP's sub-arena; bias follows its kernel
__host__ __device__ inline int64_t leaf_kernel_off(int l, int deg) {
  int64_t off = 0;
  for (int i = 0; i < l; ++i) off += (int64_t)layer_in(i) * layer_out(i, deg) + layer_out(i, deg);
  return off;
}
__host__ __device__ inline int64_t leaf_bias_off(int l, int deg) {
  return leaf_kernel_off(l, deg) + (int64_t)layer_in(l) * layer_out(l, deg);
}
__host__ __device__ inline int64_t mlp_param_count(int deg) { return leaf_kernel_off(10, deg); }

// ---- packed (MFMA fragment order) weight images --------------------------------------
// A packed matrix B[K][N] (K = 8*KG, N = 32*NCB) stores element (k,n) at
//   ((g*NCB + c)*64 + lane)*4 + j,  g=k/8, lane=((k%8)/4)*32 + n%32, j=k%4, c=n/32
// so that one wave reads a (k-group, col-block) fragment as 64 lanes x 16 B contiguous and
// lane l feeds mfma_f32_32x32x2f32 number j with B[k=8g+4*(l>>5)+j][n=32c+(l&31)].
__host__ __device__ inline int64_t packed_index(int k, int n, int ncb) {
  int g = k >> 3, kk = k & 7;
  int lane = ((kk >> 2) << 5) | (n & 31);
  return (((int64_t)g * ncb + (n >> 5)) * 64 + lane) * 4 + (kk & 3);
}

// forward image: trunk layer l (0..7) then heads then biases
__host__ __device__ inline int fwd_kgroups(int l) { return l == 0 ? 8 : (l == 5 ? 40 : 32); }
__host__ __device__ inline int64_t fwd_layer_off(int l) {  // l in 0..8 (8 = heads)
  int64_t off = 0;
  for (int i = 0; i < l; ++i) off += (int64_t)fwd_kgroups(i) * 8 * 256;
  return off;
}
__host__ __device__ inline int64_t fwd_bias_off(int deg) {
  return fwd_layer_off(8) + (int64_t)32 * head_blocks(deg) * 256;
}
__host__ __device__ inline int64_t fwd_image_floats(int deg) {
  return fwd_bias_off(deg) + 8 * kW + 32 * head_blocks(deg);
}
// backward(data) image: head^T (K = 32*NHB, N = 256), then W_l^T for l = 7..1 (K = 256 outputs,
// N = first 256 inputs)
__host__ __device__ inline int64_t bwd_layer_off(int l, int deg) {  // l in 1..7
  return (int64_t)head_blocks(deg) * 32 * 256 + (int64_t)(7 - l) * 256 * 256;
}
__host__ __device__ inline int64_t bwd_image_floats(int deg) { return bwd_layer_off(0, deg); }

// ---- bf16x6 images (mlp_x6_kernels.hip; PxoCfg.mlp_precision = PXO_MLP_BF16X6) ---------------------------------------
// Every weight is split into three bf16 parts w = w1 + w2 + w3; a (16-deep k-group, 32-column block) is stored as three
// fragments [w1 | w2 | w3] of 64 lanes x 16 B (8 bf16: k = 16 kg + 8 (lane >> 5) + e, column 32 cb + (lane & 31)).
// Offsets below are in 4-byte slots, like the float32 images'.
constexpr int kX6KgSlots = 8 * 3 * 256;       // slots per k-group of a 256-column layer
__host__ __device__ inline int x6_fwd_kg(int l) { return l == 0 ? 4 : (l == 5 ? 20 : 16); }
__host__ __device__ inline int64_t x6_fwd_layer_off(int l) {  // l in 0..8 (8 = heads)
  int64_t off = 0;
  for (int i = 0; i < l; ++i) off += (int64_t)x6_fwd_kg(i) * kX6KgSlots;
  return off;
}
__host__ __device__ inline int64_t x6_fwd_bias_off(int deg) {
  return x6_fwd_layer_off(8) + (int64_t)16 * head_blocks(deg) * 3 * 256;
}
__host__ __device__ inline int64_t x6_fwd_image_floats(int deg) {
  return x6_fwd_bias_off(deg) + 8 * kW + 32 * head_blocks(deg);
}
// backward(data): head^T (K = the head columns, zero-padded to whole groups of 4 k-groups), then W_l^T for l = 7..1
__host__ __device__ inline int x6_bwd_head_kg(int deg) { return 4 * ((head_blocks(deg) + 1) / 2); }
__host__ __device__ inline int64_t x6_bwd_image_floats(int deg) {
  return (int64_t)(x6_bwd_head_kg(deg) + 7 * 16) * kX6KgSlots;
}

__host__ __device__ inline int64_t num_tiles(int64_t M) { return (M + kTM - 1) / kTM; }

// Tile schedule of one fused-MLP launch over M rows on `grid` persistent workgroups (the same function of (M, grid)
// in the forward and the backward(data) kernel): whole rounds of full 128-row tiles; if the rows that are left fit
// into ONE round at half height they are cut into 64-row tiles (one per workgroup, 2 of the 4 row blocks), so the
// ragged last round costs about half a tile time instead of a whole one (4096 rays x 192 samples + 10,000 sparsity
// points = 24 full rounds + 157 half tiles on 256 CUs, instead of 25 rounds).  Tile t lives in mask/partial slot t;
// half tile h in slot n_full + h.
struct TileSched {
  int64_t n_full;      // full tiles: rows [t*128, t*128+128)
  int64_t n_half;      // half tiles: rows [half_row0 + h*64, +64)
  int64_t half_row0;
};
__host__ __device__ inline TileSched tile_sched(int64_t M, int64_t grid) {
  TileSched t;
  const int64_t tiles = num_tiles(M);
  t.n_full = tiles; t.n_half = 0; t.half_row0 = tiles * kTM;
  if (grid < 1 || tiles <= grid) return t;
  const int64_t whole = (tiles / grid) * grid;
  const int64_t left = M - whole * kTM;             // > 0 rows after the whole rounds (0 if tiles % grid == 0 and M % 128 == 0)
  if (left > 0 && left <= grid * (kTM / 2)) {
    t.n_full = whole;
    t.half_row0 = whole * kTM;
    t.n_half = (left + kTM / 2 - 1) / (kTM / 2);
  }
  return t;
}
// relu-mask image written by the forward kernel: per (slot, layer, thread) kMaskWords words
__host__ __device__ inline int64_t mask_slots(int64_t M) { return num_tiles(M) + kMaxMlpGrid / 2; }
__host__ __device__ inline int64_t mask_words(int64_t M) {
  return mask_slots(M) * kDepth * kMlpThreads * kMaskWords;
}
// bias-gradient partials written by the backward-data kernel, one per TILE SLOT: [slot][9][256] (a tile's column sums do
// not depend on which workgroup computed it, so any tile schedule gives the same bits), + one live byte per slot behind
__host__ __device__ inline int64_t dbias_floats(int64_t M) { return mask_slots(M) * (9 * kW + 1); }
__host__ __device__ inline const uint8_t* dbias_tile_live(const float* dbias_partial, int64_t M) {
  return reinterpret_cast<const uint8_t*>(dbias_partial + mask_slots(M) * 9 * kW);
}

// ---- error plumbing ------------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);

#define PXO_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      pxo::set_error(__VA_ARGS__);        \
      return PXO_ERR_ARG;                 \
    }                                     \
  } while (0)

int validate_cfg(const PxoCfg* cfg);
int num_cus();
unsigned mlp_grid(int64_t M);      // persistent workgroups of a float32 / bf16x6 fused-MLP launch over M rows (mlp_kernels.hip)
int mlp_bwd_partials(int64_t M);   // number of [9][256] tile partials (slots) mlp_bwd_data writes for M rows: tile_sched(M, mlp_grid(M))

// HIP-event bracket around one kernel launch (active for the tags in pxo_profile_enable's mask)
struct KernelTimer {
  KernelTimer(int tag, int64_t rows, hipStream_t s);
  ~KernelTimer();
  int slot;
  hipStream_t stream;
};
int launch_mlp_fwd_grid(const PxoCfg* cfg, const float* packed_fwd, int reso, int x0, int x1,
                        const float* off, const float* scale, float* sigma_out, hipStream_t s);

// ---- launchers implemented in the kernel translation units -----------------------------
int launch_pack(const PxoCfg* cfg, const float* mlp_params, float* fwd, float* bwd, hipStream_t s);
// tile_counter (may be NULL = static tile stride): a ZERO device word; the persistent workgroups of the training
// instantiation then take their tiles from it (pxo_mlp.h TileTicket)
int launch_mlp_fwd(const PxoCfg* cfg, const float* packed_fwd, const float* pts, int64_t M,
                   float* raw_rgb, float* raw_sigma, float* acts, float* enc, uint32_t* mask,
                   hipStream_t s, unsigned int* tile_counter = nullptr);
// chunk_live (may be NULL = dense): one byte per kLiveRows rows, WRITTEN by the backward(data) kernel (1: some row of the
// chunk has a non-zero upstream gradient) and READ by the weight-gradient kernels, which skip dead chunks
__host__ __device__ inline int64_t live_flags(int64_t M) { return (M + kLiveRows - 1) / kLiveRows + kTM / kLiveRows; }
// tile_counter (may be NULL = static tile stride): a ZERO device word (the train step's first launch zeroes them); the
// persistent workgroups then TAKE tiles from it instead of striding over them (skipped tiles do not leave workgroups idle; a
// late-starting workgroup is not the tail).
// bias_from_wgrad (bf16x6 with its own weight-gradient kernel only; the train step passes the same value to BOTH launches of a
// pass): the bias gradients of Dense_1..7 are the column sums of dz_1..7 that wgrad_x6_kernel takes while it streams dz --
// backward(data) then skips its per-layer lane reductions for those layers (6 % of its time) and the reduce reads the
// per-range sums instead of the per-slot partials.
int launch_mlp_bwd_data(const PxoCfg* cfg, const float* packed_bwd, const float* d_raw_rgb,
                        const float* d_raw_sigma, const uint32_t* mask, int64_t M, float* dz,
                        float* dbias_partial, uint8_t* chunk_live, unsigned int* tile_counter, hipStream_t s,
                        bool bias_from_wgrad);

// ---- run-time choices between implementations of the same result (pxo_set_tuning; A/B sessions and equality tests) ----
// An entry point takes ONE snapshot of the knobs (pxo_api.hip tuning_snapshot) and passes what it decided from it down; no
// function below the entry points reads a knob.
struct Tuning {
  int tile_sched;             // PXO_TUNE_TILE_SCHED: 0 static stride, 1 device counter (dense training kernels)
  int wgrad_ranges;           // PXO_TUNE_WGRAD_RANGES: 0 = built-in choice, n > 0 = row ranges per layer of the 256x256 products
  int wgrad_skinny_ranges;    // PXO_TUNE_WGRAD_SKINNY_RANGES: the same for the enc-based pair and the head product
  int coarse_stream;          // PXO_TUNE_COARSE_REVERSE_STREAM: 1 = the coarse reverse pass on a side stream
  int x6_wgrad;               // PXO_TUNE_X6_WGRAD: 1 = in bf16x6 the 256x256 weight gradients run on the bf16 pipe too, 0 = float32 MFMA
  int vd_ray_block;           // PXO_TUNE_VD_RAY_BLOCK: rays per internal block of pxo_vd_render_fwd
};
Tuning tuning_snapshot();     // pxo_api.hip: every knob, read once

constexpr int kKC = 32;           // row granularity of the weight-gradient split (rows_per_wg is a multiple of it)
// The split of a pass of M rows over `ncu` CUs: row ranges per layer of the 256x256 products / of the skinny products.
//  * big passes (>= 1024 rows per CU): one range per CU and layer (NL whole waves of workgroups on the 2 ncu slots);
//  * smaller ones: 4 ncu / NL ranges (4 waves) -- round 3, rays/s at 4096 / 1024 / 512 rays per step on 256 CUs:
//    256 ranges 161.0 k / 141.6 k / 123.6 k, 146 ranges 156.5 k / 144.3 k / 127.9 k (one launch per layer: 159.7 k /
//    139.9 k / 120.3 k): long ranges lose on big passes (the two column halves drift apart and the shared operand stops
//    hitting L2), short ones pay 64 MB of slab traffic per layer;
//  * the skinny products run two workgroups per CU: 2 ncu ranges, ncu below 512 rows per CU (round 3, ms per step
//    at 512 / 1024 / 4096 rays: 512 ranges 3.732 / 6.686 / 24.19, 256 ranges 3.716 / 6.689 / 24.28, 384: 3.739 / 6.722 /
//    24.41, 128: slower).
// Tuning::wgrad_ranges / wgrad_skinny_ranges override either (A/B sessions).
struct WgradSplit { int64_t rpw_main; int P_main; int64_t rpw_skinny; int P_skinny; };
inline void split_rows(int64_t M, int64_t target, int64_t* rows_per_wg, int* P) {
  int64_t rpw = (M + target - 1) / target;
  rpw = (rpw + kKC - 1) / kKC * kKC;
  if (rpw < kKC) rpw = kKC;
  *rows_per_wg = rpw;
  *P = (int)((M + rpw - 1) / rpw);
}
inline WgradSplit wgrad_split(int64_t M, int ncu, const Tuning& tu) {
  constexpr int NL = kDepth - 1;
  WgradSplit w;
  int ranges = M >= (int64_t)1024 * ncu ? ncu : (4 * ncu / NL > 0 ? 4 * ncu / NL : 1);
  if (tu.wgrad_ranges > 0) ranges = tu.wgrad_ranges;
  if (ranges > ncu) ranges = ncu;
  split_rows(M, ranges, &w.rpw_main, &w.P_main);
  int skinny = M < (int64_t)512 * ncu ? ncu : 2 * ncu;
  if (tu.wgrad_skinny_ranges > 0) skinny = tu.wgrad_skinny_ranges;
  if (skinny > 2 * ncu) skinny = 2 * ncu;
  split_rows(M, skinny, &w.rpw_skinny, &w.P_skinny);
  return w;
}
// zero-row skipping needs every row range to fit a workgroup's live-chunk list
inline bool wgrad_split_fits_live_list(const WgradSplit& w) {
  return w.rpw_main <= (int64_t)kMaxLiveChunks * kLiveRows && w.rpw_skinny <= (int64_t)kMaxLiveChunks * kLiveRows;
}

// What a train step (or a standalone reverse launch) decides before its first launch, from one Tuning snapshot.
struct StepPlan {
  bool dyn;                   // the dense MLP launches take their tiles from the device counters
  WgradSplit split_c, split_f;  // weight-gradient row ranges of the coarse / fine pass (split_f: M_f = 0 without a fine level)
  bool skip;                  // skip_zero_rows, and every range of both passes fits the live lists: else the reverse pass runs
                              // dense (> 32,768 rows per range, i.e. more than 8.4 M sample rows on 256 CUs: same bits, no saving)
  bool x6_main;               // the 256x256 weight gradients on the bf16 pipe (bf16x6 with Tuning::x6_wgrad)
  bool bias_from_wgrad;       // the train step takes the bias gradients of Dense_1..7 from that kernel (launch_mlp_bwd_data)
  bool fork;                  // the coarse reverse pass on the side stream (needs a fine level)
};
inline StepPlan plan_step(const PxoCfg& cfg, int64_t M_c, int64_t M_f, int ncu, const Tuning& tu) {
  StepPlan p;
  p.dyn = tu.tile_sched != 0;
  p.split_c = wgrad_split(M_c, ncu, tu);
  p.split_f = wgrad_split(M_f, ncu, tu);
  p.skip = cfg.skip_zero_rows != 0 && wgrad_split_fits_live_list(p.split_c) &&
           (M_f == 0 || wgrad_split_fits_live_list(p.split_f));
  p.x6_main = cfg.mlp_precision == PXO_MLP_BF16X6 && tu.x6_wgrad != 0;
  p.bias_from_wgrad = p.x6_main;
  p.fork = M_f > 0 && tu.coarse_stream != 0;
  return p;
}

// wgrad_x6_kernels.hip: the 256x256 products of Dense_1..7 in bf16x6 (same grid, slabs and reduce as the float32 launch)
void launch_wgrad_main_x6(const float* acts, const float* dz1, int64_t M, int64_t rpw, int P, float* slab, int n_layers,
                          int64_t layer_stride, const uint8_t* chunk_live, float* dz_colsum, hipStream_t s);
size_t wgrad_workspace_bytes(const PxoCfg* cfg, int64_t M);
// split: the caller's (wgrad_split of this M); chunk_live only with a split that fits the live lists (StepPlan::skip);
// bias_from_wgrad only with x6_main (StepPlan)
int launch_mlp_bwd_weights(const PxoCfg* cfg, const float* acts, const float* enc, const float* dz,
                           const float* d_raw_rgb, const float* d_raw_sigma,
                           const float* dbias_partial, int64_t M, float* grads, void* ws,
                           size_t ws_bytes, const uint8_t* chunk_live, hipStream_t s, const WgradSplit& split,
                           bool x6_main, bool bias_from_wgrad);
int launch_count_live(const uint8_t* chunk_live, int64_t n, unsigned long long* out, hipStream_t s);
int launch_posenc(const float* x, int64_t N, float* enc, hipStream_t s);
// opt-in split-precision forward (mlp_x3_kernels.hip); pts == nullptr selects the dense-grid point source
int launch_pack_x3(const PxoCfg* cfg, const float* mlp_params, float* fwd, hipStream_t s);
int launch_mlp_fwd_x3(const PxoCfg* cfg, const float* packed_fwd, const float* pts, int reso, int x0, const float* off,
                      const float* scale, int64_t M, float* raw_rgb, float* raw_sigma, hipStream_t s);

// opt-in float32-accurate split-precision training kernels (mlp_x6_kernels.hip); pts == nullptr selects the dense-grid source
int launch_pack_x6(const PxoCfg* cfg, const float* mlp_params, float* fwd, float* bwd, hipStream_t s);
int launch_mlp_fwd_x6(const PxoCfg* cfg, const float* packed_fwd, const float* pts, int reso, int x0, const float* off,
                      const float* scale, int64_t M, float* raw_rgb, float* raw_sigma, float* acts, float* enc,
                      uint32_t* mask, unsigned int* tile_counter, hipStream_t s);
int launch_mlp_bwd_data_x6(const PxoCfg* cfg, const float* packed_bwd, const float* d_raw_rgb, const float* d_raw_sigma,
                           const uint32_t* mask, int64_t M, float* dz, float* dbias_partial, uint8_t* chunk_live,
                           unsigned int* tile_counter, hipStream_t s, bool db_all = true);

int launch_sample_along_rays(const float* o, const float* d, int64_t B, int S, float near_,
                             float far_, int lindisp, const float* t_rand, float* z, float* pts,
                             hipStream_t s);
int launch_shade_composite_fwd(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma,
                               const float* z, const float* dirs, const float* viewdirs, int64_t B,
                               int S, float* comp_rgb, float* disp, float* acc, float* weights,
                               hipStream_t s, const float* lobes = nullptr);   // lobes [K,4]: the NeRF-SG basis instead of SH
int launch_shade_composite_bwd(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma,
                               const float* z, const float* dirs, const float* viewdirs,
                               const float* d_comp_rgb, int64_t B, int S, float* d_raw_rgb,
                               float* d_raw_sigma, hipStream_t s);
int launch_sample_pdf(const float* z_c, const float* w_c, const float* o, const float* d, int64_t B,
                      int Nc, int Nf, const float* u, float* z_out, float* pts, hipStream_t s);
int launch_generate_rays(const float* c2w, int n_cams, int W, int H, float focal, const int64_t* pix, int64_t B,
                         float* o, float* d, float* v, hipStream_t s);
int launch_sample_batch(uint64_t seed, uint64_t stream_id, const float* c2w, int W, int H, float focal, const float* image,
                        int64_t B, int64_t first, int64_t* ids, float* o, float* d, float* v, float* pixels, hipStream_t s);
int launch_generate_rays_ndc(const float* c2w, int n_cams, int W, int H, float focal, float near, const int64_t* pix, int64_t B,
                             float* o, float* d, float* v, hipStream_t s);
int launch_sample_batch_ndc(uint64_t seed, uint64_t stream_id, const float* c2w, int W, int H, float focal, float near,
                            const float* image, int64_t B, int64_t first, int64_t* ids, float* o, float* d, float* v,
                            float* pixels, hipStream_t s);
int launch_randint(uint64_t seed, uint64_t stream_id, int64_t count, int64_t n, int64_t* out, hipStream_t s);
int launch_mean_samples(const float* raw_rgb, const float* raw_sigma, int64_t n_cells, int S, int C, float* out,
                        hipStream_t s);
int launch_uniform(uint64_t seed, uint64_t stream_id, int64_t n, float lo, float hi, float* out,
                   hipStream_t s);
// first: raw[i] takes the draw of element first + i of the stream (a block of a larger batch)
int launch_add_noise(float* raw, int64_t n, float noise_std, const float* noise, uint64_t seed, uint64_t stream_id, hipStream_t s,
                     int64_t first = 0);
// compositing of the view-conditioned head (render_kernels.hip vd_composite_fwd_kernel); weights may be NULL
int launch_vd_composite_fwd(int white_bkgd, const float* raw_rgb, const float* raw_sigma, const float* z, const float* dirs,
                            int64_t B, int S, float* comp_rgb, float* disp, float* acc, float* weights, hipStream_t s);
int launch_adam(float* p, float* m, float* v, const float* g, int64_t n, float lr, int64_t step,
                float grad_scale, hipStream_t s);
// training form of the compositing: forward + pixel loss + reverse in one launch (see render_kernels.hip); serves the
// n_sp sparsity rows appended to the pass as well.  With lobes [K,4] and lobe_partials [sg_ray_blocks(B)][K][4] it is the NeRF-SG
// form: the basis from the lobes, and the per-workgroup partials of the lobe gradient; both NULL is the SH form
__host__ __device__ inline int64_t sg_ray_blocks(int64_t B) { return (B + PXO_SG_RAYS_PER_BLOCK - 1) / PXO_SG_RAYS_PER_BLOCK; }
int launch_shade_composite_train(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, const float* z,
                                 const float* dirs, const float* viewdirs, const float* pixels, int64_t B, int S,
                                 float* comp_rgb, float* weights, float* ray_sse, float* d_raw_rgb, float* d_raw_sigma,
                                 int64_t n_sp, float* sp_exp, const float* lobes, float* lobe_partials, hipStream_t s);
// sg_params [3K] -> lobes [K,4], and the fixed-order second stage of the lobe gradient (partials of up to two passes; see the
// kernels' comments for d_lobes / sg_grads / sumsq_slot, each of which may be NULL)
int launch_sg_lobes(const float* sg_params, int K, float* lobes, hipStream_t s);
int launch_sg_lobe_grad(const float* part_a, int64_t nb_a, const float* part_b, int64_t nb_b, int K, const float* sg_params,
                        float wd_coef, float* d_lobes, float* sg_grads, float* sumsq_slot, hipStream_t s);
// up to 3 uniform draws (Philox streams of one seed) in one launch
struct UniformJob { uint64_t stream_id; int64_t n; float lo, hi; float* out; };
// sq_x != NULL: the same launch also writes the kSumsqBlocks fixed-order partial sums of squares of sq_x[0 .. sq_n) (the
// parameter norm of weight_l2, train.py:101-108: it depends on the parameters only, so it rides with the step's first launch)
constexpr int kSumsqBlocks = 64;
// step_words != NULL: the same launch also writes n_words (<= 256) device words, step_words[0] = first_word and the rest zero
// (the train step's record and the tile counters of its MLP launches)
int launch_uniform_jobs(uint64_t seed, const UniformJob* jobs, int n_jobs, hipStream_t s, const float* sq_x = nullptr,
                        int64_t sq_n = 0, float* sq_partial = nullptr, unsigned int* step_words = nullptr, int n_words = 0,
                        unsigned int first_word = 0);
int launch_finalize_stats(const float* sse_f, const float* sse_c, const float* sp_exp, const float* sumsq_partial,
                          int64_t B, int64_t n_sp, float sp_weight, int64_t n_params, float* stats, hipStream_t s);
int launch_adam_pack(const PxoCfg* cfg, float* p, float* m, float* v, const float* g, float lr, int64_t step,
                     float grad_scale, float* fwd0, float* bwd0, float* fwd1, float* bwd1, hipStream_t s);
// occupancy_kernels.hip: the checks of a PxoOccGrid (`who` opens the message), and the cull / expand passes without them
int occ_validate(const PxoOccGrid* occ, const char* who);
size_t occ_cull_workspace_bytes(int64_t M);
int launch_occ_cull(const PxoOccGrid& occ, const float* pts, int64_t M, float* pts_live, int32_t* slot, int64_t* n_live_dev,
                    void* ws, hipStream_t s);
int launch_occ_expand(const float* rgb_live, const float* sigma_live, const int32_t* slot, int64_t M, int C, float* raw_rgb,
                      float* raw_sigma, hipStream_t s);
// the reverse of launch_occ_expand (rows with slot < 0 dropped), and slot[i] = first + i for rows that are always live
int launch_occ_gather(const float* d_rgb, const float* d_sigma, const int32_t* slot, int64_t M, int C, float* d_rgb_live,
                      float* d_sigma_live, hipStream_t s);
int launch_occ_tail_slots(int32_t* slot, int64_t n, int64_t first, hipStream_t s);
int launch_fill(float* p, int64_t n, float v, hipStream_t s);
int launch_axpy(float* y, const float* x, int64_t n, float a, hipStream_t s);

}  // namespace pxo
