// C ABI of the gfx950 NeRF-SH hot path (see include/plenoctree_hip.h).  Host-side glue only:
// argument checks, workspace carving and the kernel sequences of NerfModel.__call__
// (nerf_sh/nerf/models.py:216-348) and loss_fn/value_and_grad (nerf_sh/train.py:66-116).
// Each sequence is written once: lay_out carves every workspace, level_forward / level_reverse launch one level of NeRF,
// render_fwd_impl / train_fwd_bwd_impl order them.  The SH, NeRF-SG and culled entry points are thin callers that differ in what
// they pass: SG lobes, an occupancy grid (the cull context), both or neither.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pxo_common.h"

namespace pxo {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return PXO_ERR_HIP;
  }
  return PXO_OK;
}

int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
    if (2 * n > kMaxMlpGrid) n = kMaxMlpGrid / 2;
  }
  return n;
}

// run-time choices between implementations of the same result (pxo_set_tuning)
// tile schedule: the device counter by default (r05b: 3.548 vs 3.556 ms per step at 512 rays, 23.78 vs 23.84 at 4096 in one
// process, profiles/r05b_tune_ab.jsonl; and a workgroup that starts late is not the launch's tail, r05b_contention_probe.jsonl)
// (atomics: a knob may be set from one host thread while another enqueues a step; an entry point reads them all ONCE, through
// tuning_snapshot, and passes down what it decided from that snapshot -- pxo_common.h StepPlan)
static std::atomic<int> g_tune_tile_sched{1};
static std::atomic<int> g_tune_wgrad_ranges{0};
static std::atomic<int> g_tune_wgrad_skinny_ranges{0};
static std::atomic<int> g_tune_x6_wgrad{1};
// PXO_TUNE_COARSE_REVERSE_STREAM: 1 = the reverse pass of the coarse level (backward(data), weight gradients, slab reduce of
// MLP_0) runs on an internal side stream beside the fine level's forward, whose ragged last round of tiles leaves CUs idle
// (3.3 rounds at 512 rays per GPU); 0 (default) = everything on the caller's stream.  Same kernels, same sums: bits unchanged.
// Measured (r06b): 3.5905 / 3.5849 vs 3.5909 / 3.5969 ms per 512-ray step, 23.56 vs 23.72 ms at 4096 rays -- +0.2 % / +0.7 %,
// and per-kernel HIP-event times stop meaning anything (the fine forward shares the GPU with the coarse reverse: 4.83 ms
// "per launch" instead of 3.95), so the measured default stays the single stream.
static std::atomic<int> g_tune_coarse_stream{0};
// PXO_TUNE_VD_RAY_BLOCK: rays per internal block of pxo_vd_render_fwd (viewdirs_kernels.hip); bits unchanged
static std::atomic<int> g_tune_vd_ray_block{PXO_VD_RAY_BLOCK_DEFAULT};
Tuning tuning_snapshot() {
  return Tuning{g_tune_tile_sched.load(), g_tune_wgrad_ranges.load(), g_tune_wgrad_skinny_ranges.load(),
                g_tune_coarse_stream.load(), g_tune_x6_wgrad.load(), g_tune_vd_ray_block.load()};
}

// The side stream of that mode and its fork / join events: one set per host thread and device, created on first use and kept
// for the thread's life (steps enqueued from different threads or for different devices never share them).
struct SideStream { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
static SideStream* side_stream() {
  static thread_local std::vector<SideStream> per_device;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
  if ((size_t)dev >= per_device.size()) per_device.resize(dev + 1);
  SideStream& x = per_device[dev];
  if (x.stream) return &x;
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  if (hipStreamCreateWithPriority(&x.stream, hipStreamNonBlocking, lo) != hipSuccess) { x.stream = nullptr; return nullptr; }
  if (hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess) {
    (void)hipStreamDestroy(x.stream);
    x.stream = nullptr;
    return nullptr;
  }
  return &x;
}

// The fork of the coarse reverse pass: it goes to `sc`, the side stream when `fork` and one is there (else `s`: the same kernels
// in stream order, the same bits).  join() makes `s` wait for everything enqueued on `sc` so far; the destructor joins as
// well, so that no return path leaves `s` running ahead of work still queued on the side stream.
struct SideFork {
  hipStream_t s, sc;
  SideStream* side = nullptr;
  SideFork(hipStream_t s_, bool fork) : s(s_), sc(s_) {
    SideStream* x = fork ? side_stream() : nullptr;
    if (x && hipEventRecord(x->fork, s) == hipSuccess && hipStreamWaitEvent(x->stream, x->fork, 0) == hipSuccess) {
      side = x;
      sc = x->stream;
    }
  }
  ~SideFork() { (void)join(); }
  bool join() {
    if (!side) return true;
    SideStream* x = side;
    side = nullptr;
    return hipEventRecord(x->join, sc) == hipSuccess && hipStreamWaitEvent(s, x->join, 0) == hipSuccess;
  }
};

int validate_cfg(const PxoCfg* cfg) {
  PXO_REQUIRE(cfg != nullptr, "cfg is NULL");
  PXO_REQUIRE(cfg->sh_deg >= 0 && cfg->sh_deg <= 4, "sh_deg %d not in [0,4] (nerf_sh/nerf/sh.py:69)", cfg->sh_deg);
  PXO_REQUIRE(cfg->min_deg_point == 0 && cfg->max_deg_point == 10,
              "only min_deg_point=0,max_deg_point=10 is built (got %d,%d)", cfg->min_deg_point, cfg->max_deg_point);
  PXO_REQUIRE(cfg->num_coarse_samples >= 3 && cfg->num_coarse_samples <= 128, "num_coarse_samples %d not in [3,128]",
              cfg->num_coarse_samples);
  PXO_REQUIRE(cfg->num_fine_samples >= 0 && cfg->num_coarse_samples + cfg->num_fine_samples <= 256,
              "num_coarse_samples+num_fine_samples must be <= 256");
  PXO_REQUIRE(cfg->mlp_precision == PXO_MLP_F32 || cfg->mlp_precision == PXO_MLP_BF16X3 || cfg->mlp_precision == PXO_MLP_BF16X6,
              "mlp_precision %d unknown", cfg->mlp_precision);
  PXO_REQUIRE(cfg->noise_std >= 0.f, "noise_std %g < 0 (0 = None)", (double)cfg->noise_std);
  PXO_REQUIRE(cfg->skip_zero_rows == 0 || cfg->skip_zero_rows == 1, "skip_zero_rows %d is not 0 / 1", cfg->skip_zero_rows);
  return PXO_OK;
}

// ---- HIP-event profiler ------------------------------------------------------------------
struct ProfRecord { hipEvent_t a, b; int tag; int64_t rows; };
static unsigned g_prof_mask = 0;              // bit t set: launches tagged t are bracketed by events
static std::vector<ProfRecord> g_prof;

KernelTimer::KernelTimer(int tag, int64_t rows, hipStream_t s) : slot(-1), stream(s) {
  if (!((g_prof_mask >> tag) & 1u)) return;
  ProfRecord r;
  if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
  r.tag = tag; r.rows = rows;
  (void)hipEventRecord(r.a, s);
  g_prof.push_back(r);
  slot = (int)g_prof.size() - 1;
}
KernelTimer::~KernelTimer() {
  if (slot >= 0) (void)hipEventRecord(g_prof[slot].b, stream);
}

// bump allocator over the caller's workspace; with base == nullptr it only measures
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(reinterpret_cast<char*>(b)) {}
  template <typename T>
  T* take(int64_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (size_t)count * sizeof(T);
    return p;
  }
};

struct PassBuffers {      // one MLP pass (coarse or fine)
  int64_t M = 0;          // rows through the MLP (ray samples + appended sparsity points)
  int S = 0;              // samples per ray
  float *z, *pts, *raw_rgb, *raw_sigma, *acts, *enc, *comp_rgb, *disp, *acc, *weights;
  uint32_t* mask;
  float *ray_sse, *d_raw_rgb, *d_raw_sigma, *dz, *dbias;
  uint8_t* live;          // one flag per kLiveRows rows: written by the backward(data) kernel, read by the wgrad kernels
};

static void carve_pass(Carver& c, PassBuffers& p, int64_t B, int S, int64_t extra_rows, int C, bool train,
                       bool own_outputs) {
  p.S = S;
  p.M = B * S + extra_rows;
  p.z = c.take<float>(B * S);
  p.pts = c.take<float>(p.M * 3);
  p.raw_rgb = c.take<float>(p.M * C);
  p.raw_sigma = c.take<float>(p.M);
  p.weights = c.take<float>(B * S);
  if (own_outputs) {
    p.comp_rgb = c.take<float>(B * 3);
    p.disp = c.take<float>(B);
    p.acc = c.take<float>(B);
  }
  if (train) {
    p.acts = c.take<float>(p.M * kW * kDepth);
    p.enc = c.take<float>(p.M * kEncPad);
    p.mask = c.take<uint32_t>(mask_words(p.M));
    p.ray_sse = c.take<float>(B);
    p.d_raw_rgb = c.take<float>(p.M * C);
    p.d_raw_sigma = c.take<float>(p.M);
    p.dz = c.take<float>(p.M * kW * kDepth);
    p.dbias = c.take<float>(dbias_floats(p.M));
    p.live = c.take<uint8_t>(live_flags(p.M));
  } else {
    p.acts = p.enc = p.ray_sse = p.d_raw_rgb = p.d_raw_sigma = p.dz = p.dbias = nullptr;
    p.mask = nullptr;
    p.live = nullptr;
  }
}

// The scalars block of a train workspace (128 words): [0, kSumsqBlocks) parameter-norm partials, [96, 98) the live-chunk count
// of pxo_train_backward_work, then the words the step's first launch writes (launch_uniform_jobs step_words): at 98 the step's
// record, kStepRecord | (1 if its reverse pass skipped zero rows), at [100, 104) the tile counters of its MLP launches.
constexpr int kStepWordsAt = 98;
constexpr int kStepWords = 6;
constexpr unsigned int kStepRecord = 0x5E7D5700u;
// The record of a culled step (pxo_train_fwd_bwd_culled): not kStepRecord, so that pxo_train_backward_work, whose chunk totals
// are those of the dense row count, refuses such a workspace by name.
constexpr unsigned int kStepRecordCulled = 0x5E7DC000u;

struct TrainWs {
  PassBuffers c, f;
  float *t_rand, *u, *sp, *scalars, *sp_exp;
  void* wgrad_ws;
  size_t wgrad_bytes;
  int64_t n_sp;
  size_t total;
};

static void carve_train(const PxoCfg* cfg, int64_t B, void* ws, bool train, TrainWs& t) {
  Carver c(ws);
  const int C = rgb_channels(cfg->sh_deg);
  const int Nc = cfg->num_coarse_samples, Nf = cfg->num_fine_samples;
  const bool sp = train && cfg->sparsity_weight > 0.f && cfg->sparsity_npoints > 0;
  t.n_sp = sp ? cfg->sparsity_npoints : 0;
  // eval_points_raw uses MLP_1 when there is a fine pass (nerf_sh/nerf/models.py:165-168), so the
  // sparsity points ride along as extra rows of the last pass.
  carve_pass(c, t.c, B, Nc, Nf > 0 ? 0 : t.n_sp, C, train, train);
  if (Nf > 0) carve_pass(c, t.f, B, Nc + Nf, t.n_sp, C, train, train);
  t.t_rand = c.take<float>(B * Nc);
  t.u = c.take<float>(B * (Nf > 0 ? Nf : 1));
  t.sp = c.take<float>(t.n_sp * 3 + 4);
  t.scalars = c.take<float>(128);
  t.sp_exp = c.take<float>(t.n_sp + 4);
  if (train) {
    const int64_t Mmax = Nf > 0 ? t.f.M : t.c.M;
    t.wgrad_bytes = wgrad_workspace_bytes(cfg, Mmax);
    t.wgrad_ws = c.take<char>((int64_t)t.wgrad_bytes);
  } else {
    t.wgrad_bytes = 0;
    t.wgrad_ws = nullptr;
  }
  t.total = (c.off + 255) & ~(size_t)255;
}

// What a NeRF-SG train step keeps behind the TrainWs block (whose layout and size stay those of the SH step): the lobes
// derived from sg_params and the per-workgroup partials of the lobe gradient of both levels
struct SgWs { float *lobes, *part_c, *part_f; int64_t ray_blocks; size_t total; };
static void carve_sg(const PxoCfg* cfg, int64_t B, void* ws, size_t train_total, SgWs& g) {
  Carver c(ws);
  c.off = train_total;
  const int K = sh_dim(cfg->sh_deg);
  g.ray_blocks = sg_ray_blocks(B);
  g.lobes = c.take<float>(4 * K);
  g.part_c = c.take<float>(g.ray_blocks * 4 * K);
  g.part_f = c.take<float>(g.ray_blocks * 4 * K);
  g.total = (c.off + 255) & ~(size_t)255;
}

// What a culled sequence keeps behind the TrainWs block (whose layout stays the dense sequence's): the compact points and raw
// rows of ONE level (the last level's size, sparsity points included -- t.n_sp is 0 in a render workspace; the coarse level uses
// their head), with `train` the compact upstream gradient as well, then the slots, the two counts and the cull's scratch
struct CullWs {
  float *pts_live, *rgb_live, *sigma_live, *d_rgb_live, *d_sigma_live;
  int32_t* slot;
  int64_t* n_live;
  void* cull;
  size_t total;
};
static void carve_cull(const PxoCfg* cfg, int64_t B, void* ws, const TrainWs& t, bool train, CullWs& k) {
  Carver c(ws);
  c.off = t.total;
  const int C = rgb_channels(cfg->sh_deg);
  const int64_t rows = B * (cfg->num_coarse_samples + cfg->num_fine_samples), M = rows + t.n_sp;
  k.pts_live = c.take<float>(M * 3);
  k.rgb_live = c.take<float>(M * C);
  k.sigma_live = c.take<float>(M);
  k.d_rgb_live = train ? c.take<float>(M * C) : nullptr;
  k.d_sigma_live = train ? c.take<float>(M) : nullptr;
  k.slot = c.take<int32_t>(M);
  k.n_live = c.take<int64_t>(2);
  k.cull = c.take<char>((int64_t)occ_cull_workspace_bytes(rows));
  k.total = (c.off + 255) & ~(size_t)255;
}

#define PXO_TRY(expr)            \
  do {                           \
    int _rc = (expr);            \
    if (_rc != PXO_OK) return _rc; \
  } while (0)

// Every workspace of the render and train sequences, and its size, in one place: the TrainWs block, then what a NeRF-SG step
// (`sg`) or a culled sequence (`cull`) keeps behind it.  ws == nullptr only measures (the *_workspace_bytes entry points);
// otherwise ws_bytes must hold the whole layout.  `who` names the entry point in messages.
struct Layout { TrainWs t; SgWs g; CullWs k; size_t total; };
static int lay_out(const PxoCfg* cfg, int64_t B, void* ws, size_t ws_bytes, bool train, bool sg, bool cull, const char* who,
                   Layout& L) {
  carve_train(cfg, B, ws, train, L.t);
  L.total = L.t.total;
  L.g = SgWs{nullptr, nullptr, nullptr, 0, L.total};
  if (sg) { carve_sg(cfg, B, ws, L.total, L.g); L.total = L.g.total; }
  if (cull) {                                          // the slots are int32
    const int S = cfg->num_coarse_samples + cfg->num_fine_samples;
    PXO_REQUIRE(B * (int64_t)S + L.t.n_sp < ((int64_t)1 << 31), "%s: %lld rays x %d samples exceed 2^31 rows", who, (long long)B, S);
    carve_cull(cfg, B, ws, L.t, train, L.k);
    L.total = L.k.total;
  }
  if (ws && ws_bytes < L.total) {
    set_error("%s: workspace %zu < %zu", who, ws_bytes, L.total);
    return PXO_ERR_WORKSPACE;
  }
  return PXO_OK;
}
static int workspace_bytes(const PxoCfg* cfg, int64_t B, bool train, bool sg, bool cull, const char* who, size_t* bytes) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(bytes && B >= (train ? 1 : 0), "%s: bad arguments", who);
  Layout L;
  PXO_TRY(lay_out(cfg, B, nullptr, 0, train, sg, cull, who, L));
  *bytes = L.total;
  return PXO_OK;
}

// The cull context of a sequence (optional): the grid that calls a sample live, its block of the workspace, the pinned words
// the two counts of a call land in (one pair per host thread, allocated on first use and kept for its life) and the caller's
// live_rows[2] or nullptr
struct CullCtx { const PxoOccGrid* occ; CullWs* k; int64_t* host; int64_t* live_rows; };
static int open_cull(const PxoOccGrid* occ, CullWs& k, int64_t* live_rows, const char* who, CullCtx& cx) {
  static thread_local int64_t* pinned = nullptr;
  if (!pinned && hipHostMalloc((void**)&pinned, 2 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess) pinned = nullptr;
  if (!pinned) {
    set_error("%s: hipHostMalloc of the count words failed", who);
    return PXO_ERR_HIP;
  }
  cx = CullCtx{occ, &k, pinned, live_rows};
  return PXO_OK;
}
// both culled sequences refuse density noise
static int refuse_noise(const PxoCfg* cfg, int randomized, const char* who) {
  if (randomized && cfg->noise_std > 0.f) {
    set_error("%s: noise_std > 0 with randomized sampling (noise on a culled sample's zero sigma would resurrect it)", who);
    return PXO_ERR_UNSUPPORTED;
  }
  return PXO_OK;
}
static int require_train_precision(const PxoCfg* cfg, const char* who) {
  if (cfg->mlp_precision != PXO_MLP_F32 && cfg->mlp_precision != PXO_MLP_BF16X6) {
    set_error("%s: training runs in float32 or its float32-accurate bf16x6 emulation only (mlp_precision bf16x3 is an inference option)", who);
    return PXO_ERR_UNSUPPORTED;
  }
  return PXO_OK;
}

// NerfModel.__call__ (nerf_sh/nerf/models.py:216-348) in pieces, so that the training sequence can put the reverse of the
// coarse level between the levels: the draws of the step, then level_forward / level_reverse per level.
struct Draws { const float* t_rand; const float* u; bool noisy; uint64_t seed; };

// every uniform draw of the step in one launch (jax.random.uniform call sites model_utils.py:135,262, train.py:79)
static int prepare_draws(const PxoCfg* cfg, TrainWs& t, int64_t B, int randomized, const float* t_rand, const float* u,
                         const float* sp_points, uint64_t seed, hipStream_t s, Draws& out, const float* params = nullptr,
                         int64_t n_params = 0, float* sumsq_partial = nullptr, unsigned int* step_words = nullptr,
                         int n_words = 0, unsigned int first_word = 0) {
  const int Nc = cfg->num_coarse_samples, Nf = cfg->num_fine_samples;
  PassBuffers& last = Nf > 0 ? t.f : t.c;
  UniformJob jobs[3];
  int nj = 0;
  if (randomized && !t_rand) { jobs[nj++] = UniformJob{0, B * Nc, 0.f, 1.f, t.t_rand}; t_rand = t.t_rand; }
  if (randomized && Nf > 0 && !u) { jobs[nj++] = UniformJob{1, B * Nf, 0.f, 1.f, t.u}; u = t.u; }
  if (!randomized) { t_rand = nullptr; u = nullptr; }
  if (t.n_sp > 0) {
    float* dst = last.pts + B * last.S * 3;
    if (sp_points) {
      if (hipMemcpyAsync(dst, sp_points, (size_t)t.n_sp * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("hipMemcpyAsync(sp_points) failed");
        return PXO_ERR_HIP;
      }
    } else {
      jobs[nj++] = UniformJob{2, t.n_sp * 3, -cfg->sparsity_radius, cfg->sparsity_radius, dst};
    }
  }
  out.t_rand = t_rand; out.u = u;
  out.noisy = randomized != 0 && cfg->noise_std > 0.f;     // (noise_std is not None) and randomized, model_utils.py:329
  out.seed = seed;
  return launch_uniform_jobs(seed, jobs, nj, s, params, n_params, sumsq_partial, step_words, n_words, first_word);
}

// One level of NeRF, forward: the sampling launch of the level (0 coarse, 1 fine), the MLP stage, the density noise when
// dr.noisy (models.py:258-264 / :318-324), and the training (pixels != nullptr) or inference shade + composite launch.  What
// differs between the levels is data: the level's buffers, the noise stream (3 / 4), whether a next level needs its weights,
// and whether the sparsity rows ride along (they do with the last level, eval_points_raw uses its MLP).
// The MLP stage is the fused forward on p.pts, or with a cull context: cull the B * p.S sample rows, read the live count
// (synchronises), append the always-live rows behind the live samples (the sparsity points: p.M - B * p.S of them), the same
// forward on the compact rows -- acts / enc / mask in compact order when the pass saves them -- and expand.  *M_run: the rows
// the level's MLP launches ran on.  With lobes (NeRF-SG): the lobe basis, and the partials of the lobe gradient.
static int level_forward(const PxoCfg* cfg, TrainWs& t, int level, const float* packed_fwd, const float* o, const float* d,
                         const float* v, int64_t B, const Draws& dr, const float* pixels, float* rgb, float* disp, float* acc,
                         hipStream_t s, unsigned int* tile_counter, const float* lobes, float* lobe_partials, const CullCtx* cx,
                         const char* who, int64_t* M_run = nullptr) {
  const int Nc = cfg->num_coarse_samples, Nf = cfg->num_fine_samples;
  const bool last = level == 1 || Nf == 0;
  PassBuffers& p = level == 0 ? t.c : t.f;
  if (level == 0)
    PXO_TRY(launch_sample_along_rays(o, d, B, Nc, cfg->near_, cfg->far_, cfg->lindisp, dr.t_rand, p.z, p.pts, s));
  else
    PXO_TRY(launch_sample_pdf(t.c.z, t.c.weights, o, d, B, Nc, Nf, dr.u, p.z, p.pts, s));
  int64_t M = p.M;
  if (!cx) {
    PXO_TRY(launch_mlp_fwd(cfg, packed_fwd, p.pts, M, p.raw_rgb, p.raw_sigma, p.acts, p.enc, p.mask, s, tile_counter));
  } else {
    CullWs& k = *cx->k;
    const int64_t rows = B * p.S, extra = p.M - rows;
    PXO_TRY(launch_occ_cull(*cx->occ, p.pts, rows, k.pts_live, k.slot, k.n_live + level, k.cull, s));
    if (hipMemcpyAsync(cx->host + level, k.n_live + level, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      set_error("%s: reading the live-row count: %s", who, hipGetErrorString(hipGetLastError()));
      return PXO_ERR_HIP;
    }
    const int64_t n_live = cx->host[level];
    if (n_live < 0 || n_live > rows) {
      set_error("%s: live-row count %lld outside [0, %lld]", who, (long long)n_live, (long long)rows);
      return PXO_ERR_HIP;
    }
    if (extra > 0) {                                    // slot[rows + j] = n_live + j <= p.M - 1: inside the compact arrays
      if (hipMemcpyAsync(k.pts_live + 3 * n_live, p.pts + 3 * rows, (size_t)extra * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) !=
          hipSuccess) {
        set_error("%s: hipMemcpyAsync(sparsity points) failed", who);
        return PXO_ERR_HIP;
      }
      PXO_TRY(launch_occ_tail_slots(k.slot + rows, extra, n_live, s));
    }
    M = n_live + extra;
    if (M > 0) PXO_TRY(launch_mlp_fwd(cfg, packed_fwd, k.pts_live, M, k.rgb_live, k.sigma_live, p.acts, p.enc, p.mask, s, tile_counter));
    PXO_TRY(launch_occ_expand(k.rgb_live, k.sigma_live, k.slot, p.M, rgb_channels(cfg->sh_deg), p.raw_rgb, p.raw_sigma, s));
    if (cx->live_rows) cx->live_rows[level] = n_live;
  }
  if (M_run) *M_run = M;
  if (dr.noisy) PXO_TRY(launch_add_noise(p.raw_sigma, B * p.S, cfg->noise_std, nullptr, dr.seed, 3 + level, s));
  if (pixels)
    return launch_shade_composite_train(cfg, p.raw_rgb, p.raw_sigma, p.z, d, v, pixels, B, p.S, nullptr, last ? nullptr : p.weights,
                                        p.ray_sse, p.d_raw_rgb, p.d_raw_sigma, last ? t.n_sp : 0, t.sp_exp, lobes, lobe_partials, s);
  return launch_shade_composite_fwd(cfg, p.raw_rgb, p.raw_sigma, p.z, d, v, B, p.S, rgb, disp, acc, p.weights, s, lobes);
}

// One level of NeRF, reverse: backward(data), then the weight gradients into `grads` (the level's MLP's), of the M rows the
// level's MLP ran on, on stream `s`.  Dense: M = p.M and the upstream gradient is the shade launch's d_raw_*.  Culled (k): that
// gradient gathered to compact order first; no live row, no MLP launch and a zero gradient.  The weight gradients wait for
// `join` (the fine level's: the slabs are the forked coarse pass's until then).
// The split is that of the M the launches run on; for the dense M it is plan.split_c / plan.split_f, which plan_step derives
// from the same call.  skip_zero_rows (plan.skip): rows with an exactly zero upstream gradient are left out (bit-identical).
static int level_reverse(const PxoCfg* cfg, TrainWs& t, PassBuffers& p, const float* packed_bwd, int64_t M, float* grads,
                         const StepPlan& plan, const Tuning& tu, unsigned int* tile_counter, hipStream_t s, const CullWs* k,
                         SideFork* join, const char* who) {
  const float *d_rgb = p.d_raw_rgb, *d_sigma = p.d_raw_sigma;
  if (k) {
    if (M == 0) return launch_fill(grads, mlp_param_count(cfg->sh_deg), 0.f, s);
    PXO_TRY(launch_occ_gather(d_rgb, d_sigma, k->slot, p.M, rgb_channels(cfg->sh_deg), k->d_rgb_live, k->d_sigma_live, s));
    d_rgb = k->d_rgb_live;
    d_sigma = k->d_sigma_live;
  }
  uint8_t* const live = plan.skip ? p.live : nullptr;
  PXO_TRY(launch_mlp_bwd_data(cfg, packed_bwd, d_rgb, d_sigma, p.mask, M, p.dz, p.dbias, live, tile_counter, s, plan.bias_from_wgrad));
  if (join && !join->join()) {
    set_error("%s: join of the side stream failed", who);
    return PXO_ERR_HIP;
  }
  return launch_mlp_bwd_weights(cfg, p.acts, p.enc, p.dz, d_rgb, d_sigma, p.dbias, M, grads, t.wgrad_ws, t.wgrad_bytes, live, s,
                                wgrad_split(M, num_cus(), tu), plan.x6_main, plan.bias_from_wgrad);
}

// diagnostic: `blocks` workgroups of `threads` threads that do nothing for `micros` microseconds of the device's
// constant-rate clock (what a ring all-reduce's kernel looks like to the kernels it shares the GPU with)
__global__ void occupy_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

}  // namespace pxo

using namespace pxo;

extern "C" {

const char* pxo_last_error(void) { return g_last_error.c_str(); }
int pxo_version(void) { return PXO_ABI_VERSION; }
size_t pxo_cfg_bytes(void) { return sizeof(PxoCfg); }

int pxo_set_tuning(int knob, int value) {
  switch (knob) {
    case PXO_TUNE_TILE_SCHED:
      PXO_REQUIRE(value == 0 || value == 1, "pxo_set_tuning: tile schedule must be 0 (static stride) or 1 (device counter), got %d", value);
      g_tune_tile_sched = value;
      return PXO_OK;
    case PXO_TUNE_WGRAD_RANGES:
      PXO_REQUIRE(value >= 0 && value <= num_cus(), "pxo_set_tuning: row ranges per layer must be 0 (built-in choice) .. %d, got %d",
                  num_cus(), value);
      g_tune_wgrad_ranges = value;
      return PXO_OK;
    case PXO_TUNE_COARSE_REVERSE_STREAM:
      PXO_REQUIRE(value == 0 || value == 1, "pxo_set_tuning: coarse reverse stream must be 0 (caller's stream) or 1 (side stream), got %d", value);
      g_tune_coarse_stream = value;
      return PXO_OK;
    case PXO_TUNE_WGRAD_SKINNY_RANGES:
      PXO_REQUIRE(value >= 0 && value <= 2 * num_cus(), "pxo_set_tuning: row ranges of the skinny products must be 0 (built-in choice) .. %d, got %d",
                  2 * num_cus(), value);
      g_tune_wgrad_skinny_ranges = value;
      return PXO_OK;
    case PXO_TUNE_X6_WGRAD:
      PXO_REQUIRE(value == 0 || value == 1, "pxo_set_tuning: bf16x6 weight gradients must be 0 (float32 MFMA) or 1 (bf16x6), got %d", value);
      g_tune_x6_wgrad = value;
      return PXO_OK;
    case PXO_TUNE_VD_RAY_BLOCK:
      PXO_REQUIRE(value >= 1 && value <= PXO_VD_RAY_BLOCK_MAX, "pxo_set_tuning: rays per block of pxo_vd_render_fwd must be 1 .. %d, got %d",
                  PXO_VD_RAY_BLOCK_MAX, value);
      g_tune_vd_ray_block = value;
      return PXO_OK;
    default:
      set_error("pxo_set_tuning: unknown knob %d", knob);
      return PXO_ERR_ARG;
  }
}
int pxo_get_tuning(int knob, int* value) {
  PXO_REQUIRE(value != nullptr, "pxo_get_tuning: NULL pointer");
  switch (knob) {
    case PXO_TUNE_TILE_SCHED: *value = g_tune_tile_sched; return PXO_OK;
    case PXO_TUNE_WGRAD_RANGES: *value = g_tune_wgrad_ranges; return PXO_OK;
    case PXO_TUNE_WGRAD_SKINNY_RANGES: *value = g_tune_wgrad_skinny_ranges; return PXO_OK;
    case PXO_TUNE_COARSE_REVERSE_STREAM: *value = g_tune_coarse_stream; return PXO_OK;
    case PXO_TUNE_X6_WGRAD: *value = g_tune_x6_wgrad; return PXO_OK;
    case PXO_TUNE_VD_RAY_BLOCK: *value = g_tune_vd_ray_block; return PXO_OK;
    default: set_error("pxo_get_tuning: unknown knob %d", knob); return PXO_ERR_ARG;
  }
}
int pxo_tile_rows(void) { return kTM; }

int pxo_param_layout(const PxoCfg* cfg, PxoLeaf* leaves, int64_t* floats_per_mlp) {
  PXO_TRY(validate_cfg(cfg));
  const int deg = cfg->sh_deg;
  if (leaves) {
    for (int l = 0; l < 10; ++l) {
      leaves[2 * l] = PxoLeaf{l, 0, leaf_kernel_off(l, deg), layer_in(l), layer_out(l, deg)};
      leaves[2 * l + 1] = PxoLeaf{l, 1, leaf_bias_off(l, deg), layer_out(l, deg), 1};
    }
  }
  if (floats_per_mlp) *floats_per_mlp = mlp_param_count(deg);
  return PXO_OK;
}

int pxo_packed_sizes(const PxoCfg* cfg, int64_t* fwd_floats, int64_t* bwd_floats) {
  PXO_TRY(validate_cfg(cfg));
  const bool x6 = cfg->mlp_precision == PXO_MLP_BF16X6;
  if (fwd_floats) *fwd_floats = x6 ? x6_fwd_image_floats(cfg->sh_deg) : fwd_image_floats(cfg->sh_deg);
  if (bwd_floats) *bwd_floats = x6 ? x6_bwd_image_floats(cfg->sh_deg) : bwd_image_floats(cfg->sh_deg);
  return PXO_OK;
}

int pxo_pack_weights(const PxoCfg* cfg, const float* mlp_params, float* packed_fwd, float* packed_bwd, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(mlp_params && packed_fwd, "pxo_pack_weights: NULL pointer");
  return launch_pack(cfg, mlp_params, packed_fwd, packed_bwd, (hipStream_t)stream);
}

int pxo_sample_along_rays(const float* origins, const float* directions, int64_t B, int S, float near_, float far_,
                          int lindisp, const float* t_rand, float* z_vals, float* pts, void* stream) {
  PXO_REQUIRE(B >= 0 && S >= 1, "pxo_sample_along_rays: bad sizes B=%lld S=%d", (long long)B, S);
  if (B == 0) return PXO_OK;                   // empty input: nothing to check, nothing to launch
  PXO_REQUIRE(origins && directions && z_vals && pts, "pxo_sample_along_rays: NULL pointer");
  return launch_sample_along_rays(origins, directions, B, S, near_, far_, lindisp, t_rand, z_vals, pts,
                                  (hipStream_t)stream);
}

int pxo_posenc(const float* x, int64_t N, float* enc, void* stream) {
  if (N == 0) return PXO_OK;
  PXO_REQUIRE(N >= 0 && x && enc, "pxo_posenc: bad arguments");
  return launch_posenc(x, N, enc, (hipStream_t)stream);
}

size_t pxo_relu_mask_bytes(int64_t M) { return (size_t)mask_words(M) * sizeof(uint32_t); }
size_t pxo_dbias_partial_bytes(int64_t M) { return (size_t)dbias_floats(M) * sizeof(float); }

int pxo_mlp_fwd(const PxoCfg* cfg, const float* packed_fwd, const float* pts, int64_t M, float* raw_rgb,
                float* raw_sigma, float* acts, float* enc, void* relu_mask, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (M == 0) return PXO_OK;
  PXO_REQUIRE(M >= 0 && packed_fwd && pts && raw_sigma, "pxo_mlp_fwd: bad arguments");
  PXO_REQUIRE((acts != nullptr) == (enc != nullptr) && (acts != nullptr) == (relu_mask != nullptr),
              "pxo_mlp_fwd: acts, enc and relu_mask must be all set or all NULL");
  return launch_mlp_fwd(cfg, packed_fwd, pts, M, raw_rgb, raw_sigma, acts, enc, (uint32_t*)relu_mask,
                        (hipStream_t)stream);
}

int pxo_mlp_bwd_data(const PxoCfg* cfg, const float* packed_bwd, const float* d_raw_rgb, const float* d_raw_sigma,
                     const void* relu_mask, int64_t M, float* dz, float* dbias_partial, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (M == 0) return PXO_OK;
  PXO_REQUIRE(M >= 0 && packed_bwd && d_raw_rgb && d_raw_sigma && relu_mask && dz && dbias_partial,
              "pxo_mlp_bwd_data: bad arguments");
  return launch_mlp_bwd_data(cfg, packed_bwd, d_raw_rgb, d_raw_sigma, (const uint32_t*)relu_mask, M, dz,
                             dbias_partial, nullptr, nullptr, (hipStream_t)stream, false);
}

int pxo_wgrad_workspace_bytes(const PxoCfg* cfg, int64_t M, size_t* bytes) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(bytes && M >= 0, "pxo_wgrad_workspace_bytes: bad arguments");
  *bytes = wgrad_workspace_bytes(cfg, M > 0 ? M : 1);
  return PXO_OK;
}

int pxo_mlp_bwd_weights(const PxoCfg* cfg, const float* acts, const float* enc, const float* dz,
                        const float* d_raw_rgb, const float* d_raw_sigma, const float* dbias_partial, int64_t M,
                        float* grads, void* ws, size_t ws_bytes, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(M >= 0 && acts && enc && dz && d_raw_rgb && d_raw_sigma && dbias_partial && grads && ws,
              "pxo_mlp_bwd_weights: bad arguments");
  const StepPlan plan = plan_step(*cfg, M, 0, num_cus(), tuning_snapshot());
  return launch_mlp_bwd_weights(cfg, acts, enc, dz, d_raw_rgb, d_raw_sigma, dbias_partial, M, grads, ws, ws_bytes,
                                nullptr, (hipStream_t)stream, plan.split_c, plan.x6_main, false);
}

int pxo_shade_composite_fwd(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, const float* z_vals,
                            const float* directions, const float* viewdirs, int64_t B, int S, float* comp_rgb,
                            float* disp, float* acc, float* weights, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && raw_rgb && raw_sigma && z_vals && directions && viewdirs && comp_rgb && disp && acc && weights,
              "pxo_shade_composite_fwd: bad arguments");
  return launch_shade_composite_fwd(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, B, S, comp_rgb, disp, acc,
                                    weights, (hipStream_t)stream);
}

int pxo_shade_composite_bwd(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, const float* z_vals,
                            const float* directions, const float* viewdirs, const float* d_comp_rgb, int64_t B, int S,
                            float* d_raw_rgb, float* d_raw_sigma, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && raw_rgb && raw_sigma && z_vals && directions && viewdirs && d_comp_rgb && d_raw_rgb &&
                  d_raw_sigma,
              "pxo_shade_composite_bwd: bad arguments");
  return launch_shade_composite_bwd(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, d_comp_rgb, B, S,
                                    d_raw_rgb, d_raw_sigma, (hipStream_t)stream);
}

int pxo_shade_composite_train(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, const float* z_vals,
                              const float* directions, const float* viewdirs, const float* pixels, int64_t B, int S,
                              float* comp_rgb, float* weights, float* ray_sse, float* d_raw_rgb, float* d_raw_sigma,
                              int64_t n_sp, float* sp_exp, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && n_sp >= 0 && raw_rgb && raw_sigma && z_vals && directions && viewdirs && pixels && ray_sse &&
                  d_raw_rgb && d_raw_sigma && (n_sp == 0 || sp_exp),
              "pxo_shade_composite_train: bad arguments");
  return launch_shade_composite_train(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, pixels, B, S, comp_rgb,
                                      weights, ray_sse, d_raw_rgb, d_raw_sigma, n_sp, sp_exp, nullptr, nullptr,
                                      (hipStream_t)stream);
}

int pxo_sample_pdf(const float* z_coarse, const float* w_coarse, const float* origins, const float* directions,
                   int64_t B, int Nc, int Nf, const float* u, float* z_out, float* pts, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && z_coarse && w_coarse && origins && directions && z_out && pts, "pxo_sample_pdf: bad arguments");
  return launch_sample_pdf(z_coarse, w_coarse, origins, directions, B, Nc, Nf, u, z_out, pts, (hipStream_t)stream);
}

int pxo_uniform(uint64_t seed, uint64_t stream_id, int64_t n, float lo, float hi, float* out, void* stream) {
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(n >= 0 && out, "pxo_uniform: bad arguments");
  return launch_uniform(seed, stream_id, n, lo, hi, out, (hipStream_t)stream);
}

int pxo_add_gaussian_noise(float* raw, int64_t n, float noise_std, const float* noise, uint64_t seed, uint64_t stream_id,
                           void* stream) {
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(n >= 0 && raw && noise_std >= 0.f, "pxo_add_gaussian_noise: bad arguments");
  return launch_add_noise(raw, n, noise_std, noise, seed, stream_id, (hipStream_t)stream);
}

int pxo_randint(uint64_t seed, uint64_t stream_id, int64_t count, int64_t n, int64_t* out, void* stream) {
  if (count == 0) return PXO_OK;
  PXO_REQUIRE(count >= 0 && n >= 1 && out, "pxo_randint: bad arguments");
  return launch_randint(seed, stream_id, count, n, out, (hipStream_t)stream);
}

int pxo_generate_rays(const float* c2w, int W, int H, float focal, const int64_t* pixel_ids, int64_t B,
                      float* origins, float* directions, float* viewdirs, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && W >= 1 && H >= 1 && focal > 0.f && c2w && origins && directions && viewdirs,
              "pxo_generate_rays: bad arguments");
  return launch_generate_rays(c2w, 1, W, H, focal, pixel_ids, B, origins, directions, viewdirs, (hipStream_t)stream);
}

int pxo_sample_batch(uint64_t seed, uint64_t stream_id, const float* c2w, int W, int H, float focal, const float* image_rgb,
                     int64_t B, int64_t first, int64_t* pixel_ids, float* origins, float* directions, float* viewdirs,
                     float* pixels, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && first >= 0 && W >= 1 && H >= 1 && focal > 0.f && c2w && image_rgb && origins && directions &&
                  viewdirs && pixels,
              "pxo_sample_batch: bad arguments");
  return launch_sample_batch(seed, stream_id, c2w, W, H, focal, image_rgb, B, first, pixel_ids, origins, directions, viewdirs,
                             pixels, (hipStream_t)stream);
}

int pxo_generate_rays_multi(const float* c2w, int n_cams, int W, int H, float focal, const int64_t* ray_ids, int64_t B,
                            float* origins, float* directions, float* viewdirs, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && n_cams >= 1 && W >= 1 && H >= 1 && focal > 0.f && c2w && ray_ids && origins && directions &&
                  viewdirs,
              "pxo_generate_rays_multi: bad arguments");
  return launch_generate_rays(c2w, n_cams, W, H, focal, ray_ids, B, origins, directions, viewdirs,
                              (hipStream_t)stream);
}

int pxo_generate_rays_ndc(const float* c2w, int n_cams, int W, int H, float focal, float ndc_near, const int64_t* ray_ids,
                          int64_t B, float* origins, float* directions, float* viewdirs, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && n_cams >= 1 && W >= 1 && H >= 1 && focal > 0.f && ndc_near > 0.f && c2w && origins && directions &&
                  viewdirs && (ray_ids || B <= (int64_t)n_cams * W * H),
              "pxo_generate_rays_ndc: bad arguments");
  return launch_generate_rays_ndc(c2w, n_cams, W, H, focal, ndc_near, ray_ids, B, origins, directions, viewdirs,
                                  (hipStream_t)stream);
}

int pxo_sample_batch_ndc(uint64_t seed, uint64_t stream_id, const float* c2w, int W, int H, float focal, float ndc_near,
                         const float* image_rgb, int64_t B, int64_t first, int64_t* pixel_ids, float* origins,
                         float* directions, float* viewdirs, float* pixels, void* stream) {
  if (B == 0) return PXO_OK;
  PXO_REQUIRE(B >= 0 && first >= 0 && W >= 1 && H >= 1 && focal > 0.f && ndc_near > 0.f && c2w && image_rgb && origins &&
                  directions && viewdirs && pixels,
              "pxo_sample_batch_ndc: bad arguments");
  return launch_sample_batch_ndc(seed, stream_id, c2w, W, H, focal, ndc_near, image_rgb, B, first, pixel_ids, origins,
                                 directions, viewdirs, pixels, (hipStream_t)stream);
}

int pxo_mean_over_samples(const PxoCfg* cfg, const float* raw_rgb, const float* raw_sigma, int64_t n_cells, int S,
                          float* out, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (n_cells == 0) return PXO_OK;
  PXO_REQUIRE(n_cells >= 0 && S >= 1 && raw_rgb && raw_sigma && out, "pxo_mean_over_samples: bad arguments");
  return launch_mean_samples(raw_rgb, raw_sigma, n_cells, S, rgb_channels(cfg->sh_deg), out, (hipStream_t)stream);
}

int pxo_adam_step(float* params, float* m, float* v, const float* grads, int64_t n, float lr, int64_t step,
                  float grad_scale, void* stream) {
  if (n == 0) return PXO_OK;
  PXO_REQUIRE(n >= 0 && params && m && v && grads && step >= 0, "pxo_adam_step: bad arguments");
  return launch_adam(params, m, v, grads, n, lr, step, grad_scale, (hipStream_t)stream);
}

int pxo_render_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  return workspace_bytes(cfg, B, false, false, false, "pxo_render_workspace_bytes", bytes);
}
int pxo_render_culled_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  return workspace_bytes(cfg, B, false, false, true, "pxo_render_culled_workspace_bytes", bytes);
}

// The render sequence.  lobes != NULL: the NeRF-SG form (pxo_sg_render_fwd), only the shade/composite launches differ;
// occ != NULL: the culled form (pxo_render_fwd_culled), each level's MLP between a cull and an expand, two synchronisations
static int render_fwd_impl(const PxoCfg* cfg, const float* packed_fwd0, const float* packed_fwd1, const float* origins,
                           const float* directions, const float* viewdirs, int64_t B, int randomized, const float* t_rand,
                           const float* u, uint64_t seed, float* rgb_c, float* disp_c, float* acc_c, float* rgb_f,
                           float* disp_f, float* acc_f, void* ws, size_t ws_bytes, void* stream, const float* lobes,
                           const PxoOccGrid* occ, int64_t* live_rows, const char* who) {
  PXO_TRY(validate_cfg(cfg));
  if (B == 0) return PXO_OK;                   // an empty batch has no buffers to check
  PXO_REQUIRE(B >= 0 && packed_fwd0 && origins && directions && viewdirs && rgb_c && disp_c && acc_c && ws,
              "%s: bad arguments", who);
  if (cfg->num_fine_samples > 0)
    PXO_REQUIRE(packed_fwd1 && rgb_f && disp_f && acc_f, "%s: fine outputs/weights missing", who);
  Layout L;
  PXO_TRY(lay_out(cfg, B, ws, ws_bytes, false, false, occ != nullptr, who, L));
  CullCtx cull;
  if (occ) PXO_TRY(open_cull(occ, L.k, live_rows, who, cull));
  const CullCtx* cx = occ ? &cull : nullptr;
  hipStream_t s = (hipStream_t)stream;
  Draws dr;
  PXO_TRY(prepare_draws(cfg, L.t, B, randomized, t_rand, u, nullptr, seed, s, dr));
  PXO_TRY(level_forward(cfg, L.t, 0, packed_fwd0, origins, directions, viewdirs, B, dr, nullptr, rgb_c, disp_c, acc_c, s, nullptr,
                        lobes, nullptr, cx, who));
  if (cfg->num_fine_samples > 0)
    PXO_TRY(level_forward(cfg, L.t, 1, packed_fwd1, origins, directions, viewdirs, B, dr, nullptr, rgb_f, disp_f, acc_f, s, nullptr,
                          lobes, nullptr, cx, who));
  return PXO_OK;
}

int pxo_render_fwd(const PxoCfg* cfg, const float* packed_fwd0, const float* packed_fwd1, const float* origins,
                   const float* directions, const float* viewdirs, int64_t B, int randomized, const float* t_rand,
                   const float* u, uint64_t seed, float* rgb_c, float* disp_c, float* acc_c, float* rgb_f,
                   float* disp_f, float* acc_f, void* ws, size_t ws_bytes, void* stream) {
  return render_fwd_impl(cfg, packed_fwd0, packed_fwd1, origins, directions, viewdirs, B, randomized, t_rand, u, seed, rgb_c,
                         disp_c, acc_c, rgb_f, disp_f, acc_f, ws, ws_bytes, stream, nullptr, nullptr, nullptr, "pxo_render_fwd");
}

int pxo_sg_render_fwd(const PxoCfg* cfg, const float* lobes, const float* packed_fwd0, const float* packed_fwd1,
                      const float* origins, const float* directions, const float* viewdirs, int64_t B, int randomized,
                      const float* t_rand, const float* u, uint64_t seed, float* rgb_c, float* disp_c, float* acc_c,
                      float* rgb_f, float* disp_f, float* acc_f, void* ws, size_t ws_bytes, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(lobes, "pxo_sg_render_fwd: null lobes ([sg_dim,4] with sg_dim = (sh_deg+1)^2 = %d)",
              (cfg->sh_deg + 1) * (cfg->sh_deg + 1));
  return render_fwd_impl(cfg, packed_fwd0, packed_fwd1, origins, directions, viewdirs, B, randomized, t_rand, u, seed, rgb_c,
                         disp_c, acc_c, rgb_f, disp_f, acc_f, ws, ws_bytes, stream, lobes, nullptr, nullptr, "pxo_sg_render_fwd");
}

int pxo_render_fwd_culled(const PxoCfg* cfg, const PxoOccGrid* occ, const float* lobes, const float* packed_fwd0,
                          const float* packed_fwd1, const float* origins, const float* directions, const float* viewdirs, int64_t B,
                          int randomized, const float* t_rand, const float* u, uint64_t seed, float* rgb_c, float* disp_c,
                          float* acc_c, float* rgb_f, float* disp_f, float* acc_f, int64_t live_rows[2], void* ws, size_t ws_bytes,
                          void* stream) {
  const char* who = "pxo_render_fwd_culled";
  PXO_TRY(validate_cfg(cfg));
  PXO_TRY(occ_validate(occ, who));
  PXO_TRY(refuse_noise(cfg, randomized, who));
  if (live_rows) live_rows[0] = live_rows[1] = 0;
  return render_fwd_impl(cfg, packed_fwd0, packed_fwd1, origins, directions, viewdirs, B, randomized, t_rand, u, seed, rgb_c,
                         disp_c, acc_c, rgb_f, disp_f, acc_f, ws, ws_bytes, stream, lobes, occ, live_rows, who);
}

int pxo_train_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  return workspace_bytes(cfg, B, true, false, false, "pxo_train_workspace_bytes", bytes);
}
int pxo_sg_train_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  return workspace_bytes(cfg, B, true, true, false, "pxo_sg_train_workspace_bytes", bytes);
}
int pxo_train_culled_workspace_bytes(const PxoCfg* cfg, int64_t B, size_t* bytes) {
  return workspace_bytes(cfg, B, true, false, true, "pxo_train_culled_workspace_bytes", bytes);
}

// The train sequence; `who` names the entry point in messages.
// sg_params != nullptr: the NeRF-SG step (pxo_sg_train_fwd_bwd_bucketed) -- the shade launches take the lobe basis and leave the
// partials of the lobe gradient, sg_grads is filled at the end, and weight_l2 counts the 3K SG entries.
// occ != nullptr: the culled step (pxo_train_fwd_bwd_culled) -- both levels' MLPs, forward and reverse, run on the live rows
// only, the step's record is kStepRecordCulled, and nothing is forked (the count read-back of each level synchronises).
static int train_fwd_bwd_impl(const PxoCfg* cfg, const float* params, const float* packed_fwd0, const float* packed_bwd0,
                              const float* packed_fwd1, const float* packed_bwd1, const float* origins,
                              const float* directions, const float* viewdirs, const float* pixels, int64_t B,
                              int randomized, const float* t_rand, const float* u, const float* sp_points, uint64_t seed,
                              float* grads, float* stats, void* ws, size_t ws_bytes, void* grads0_ready, void* stream,
                              const float* sg_params, float* sg_grads, const PxoOccGrid* occ, int64_t* live_rows,
                              const char* who) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(B >= 1 && params && packed_fwd0 && packed_bwd0 && origins && directions && viewdirs && pixels && grads &&
                  stats && ws,
              "%s: bad arguments", who);
  PXO_TRY(require_train_precision(cfg, who));
  if (cfg->num_fine_samples > 0) PXO_REQUIRE(packed_fwd1 && packed_bwd1, "%s: MLP_1 images missing", who);
  hipStream_t s = (hipStream_t)stream;
  const bool sg = sg_params != nullptr;
  Layout L;
  PXO_TRY(lay_out(cfg, B, ws, ws_bytes, true, sg, occ != nullptr, who, L));
  TrainWs& t = L.t;
  const SgWs& g = L.g;
  CullCtx cull;
  if (occ) PXO_TRY(open_cull(occ, L.k, live_rows, who, cull));
  const CullCtx* cx = occ ? &cull : nullptr;
  const CullWs* k = occ ? &L.k : nullptr;
  const int deg = cfg->sh_deg;
  const int64_t n_mlp = mlp_param_count(deg);
  const int sgK = sh_dim(deg);
  const int64_t n_all = 2 * n_mlp + (sg ? 3 * sgK : 0);                     // the SG leaves are counted (train.py:101-108)
  const float wd_coef = 2.f * cfg->weight_decay_mult / (float)n_all;   // d/dp of weight_decay_mult * sum(p^2)/n (train.py:101-114)
  const int Nf = cfg->num_fine_samples;
  // everything the step decides, from one snapshot of the tuning knobs, before its first launch (a culled step takes the dense
  // step's decisions: a compact pass is no longer than the dense one, so a dense split that fits the live lists stays fitting)
  const Tuning tu = tuning_snapshot();
  const StepPlan plan = plan_step(*cfg, t.c.M, Nf > 0 ? t.f.M : 0, num_cus(), tu);
  // weight_l2 = sum(p^2) / n (train.py:101-108) depends on the parameters only: its partial sums ride in the step's first
  // launch, together with every uniform draw and the step words: the step's record (what pxo_train_backward_work reports)
  // and the tile counters of its four persistent MLP launches (forward / backward(data) of each level), zeroed -- the dense
  // kernels take their tiles from them when plan.dyn, the skipping backward always
  float* const sumsq_partial = t.scalars;
  unsigned int* const step_words = reinterpret_cast<unsigned int*>(t.scalars + kStepWordsAt);
  unsigned int* const counters = step_words + 2;
  unsigned int* const cnt_fwd_c = plan.dyn ? counters + 0 : nullptr;
  unsigned int* const cnt_fwd_f = plan.dyn ? counters + 2 : nullptr;
  unsigned int* const cnt_bwd_c = (plan.dyn || cfg->skip_zero_rows) ? counters + 1 : nullptr;
  unsigned int* const cnt_bwd_f = (plan.dyn || cfg->skip_zero_rows) ? counters + 3 : nullptr;
  Draws dr;
  PXO_TRY(prepare_draws(cfg, t, B, randomized, t_rand, u, sp_points, seed, s, dr, params, 2 * n_mlp, sumsq_partial, step_words,
                        kStepWords, cx ? kStepRecordCulled : kStepRecord | (plan.skip ? 1u : 0u)));
  if (sg) PXO_TRY(launch_sg_lobes(sg_params, sgK, g.lobes, s));
  // coarse level: forward, losses (train.py:77-98), reverse of the compositing, reverse through MLP_0.  Nothing of the fine
  // level feeds MLP_0's gradient (the fine sample positions carry no gradient, model_utils.py:286), so it is complete here
  // -- a quarter into the step -- and its all-reduce can ride under the fine level.
  int64_t M_c = 0, M_f = 0;
  PXO_TRY(level_forward(cfg, t, 0, packed_fwd0, origins, directions, viewdirs, B, dr, pixels, nullptr, nullptr, nullptr, s,
                        cnt_fwd_c, g.lobes, g.part_c, cx, who, &M_c));
  // The coarse reverse pass touches nothing the fine forward reads or writes (its own workspace slices, the MLP_0 half of
  // `grads`; the weight-gradient slabs are shared with the fine pass, which therefore waits for it): with plan.fork it runs
  // on the side stream, beside sample_pdf / the fine forward, and joins before the fine weight gradients.
  SideFork fk(s, plan.fork && !cx);
  PXO_TRY(level_reverse(cfg, t, t.c, packed_bwd0, M_c, grads, plan, tu, cnt_bwd_c, fk.sc, k, nullptr, who));
  if (cfg->weight_decay_mult != 0.f) PXO_TRY(launch_axpy(grads, params, n_mlp, wd_coef, fk.sc));
  if (grads0_ready && hipEventRecord((hipEvent_t)grads0_ready, fk.sc) != hipSuccess) {
    set_error("%s: hipEventRecord(grads0_ready) failed", who);
    return PXO_ERR_HIP;
  }
  if (Nf > 0) {
    PXO_TRY(level_forward(cfg, t, 1, packed_fwd1, origins, directions, viewdirs, B, dr, pixels, nullptr, nullptr, nullptr, s,
                          cnt_fwd_f, g.lobes, g.part_f, cx, who, &M_f));
    PXO_TRY(level_reverse(cfg, t, t.f, packed_bwd1, M_f, grads + n_mlp, plan, tu, cnt_bwd_f, s, k, &fk, who));
  } else {
    PXO_TRY(launch_fill(grads + n_mlp, n_mlp, 0.f, s));
  }
  if (cfg->weight_decay_mult != 0.f) PXO_TRY(launch_axpy(grads + n_mlp, params + n_mlp, n_mlp, wd_coef, s));
  // the lobe gradient: both levels' partials in a fixed order, back through softplus / spher2cart, plus its weight-decay term;
  // the same launch adds sum(sg_params^2) to the first parameter-norm partial
  if (sg)
    PXO_TRY(launch_sg_lobe_grad(g.part_c, g.ray_blocks, Nf > 0 ? g.part_f : nullptr, g.ray_blocks, sgK, sg_params, wd_coef,
                                nullptr, sg_grads, sumsq_partial, s));
  PXO_TRY(launch_finalize_stats(Nf > 0 ? t.f.ray_sse : nullptr, t.c.ray_sse, t.n_sp > 0 ? t.sp_exp : nullptr, sumsq_partial,
                                B, t.n_sp, cfg->sparsity_weight, n_all, stats, s));
  return PXO_OK;
}

int pxo_train_fwd_bwd_bucketed(const PxoCfg* cfg, const float* params, const float* packed_fwd0, const float* packed_bwd0,
                               const float* packed_fwd1, const float* packed_bwd1, const float* origins,
                               const float* directions, const float* viewdirs, const float* pixels, int64_t B,
                               int randomized, const float* t_rand, const float* u, const float* sp_points, uint64_t seed,
                               float* grads, float* stats, void* ws, size_t ws_bytes, void* grads0_ready, void* stream) {
  return train_fwd_bwd_impl(cfg, params, packed_fwd0, packed_bwd0, packed_fwd1, packed_bwd1, origins, directions, viewdirs,
                            pixels, B, randomized, t_rand, u, sp_points, seed, grads, stats, ws, ws_bytes, grads0_ready, stream,
                            nullptr, nullptr, nullptr, nullptr, "pxo_train_fwd_bwd");
}

// (no sg_params: a culled NeRF-SG step is not built, and the families table refuses it before this is reached)
int pxo_train_fwd_bwd_culled(const PxoCfg* cfg, const PxoOccGrid* occ, const float* params, const float* packed_fwd0,
                             const float* packed_bwd0, const float* packed_fwd1, const float* packed_bwd1, const float* origins,
                             const float* directions, const float* viewdirs, const float* pixels, int64_t B, int randomized,
                             const float* t_rand, const float* u, const float* sp_points, uint64_t seed, float* grads,
                             float* stats, void* ws, size_t ws_bytes, void* grads0_ready, void* stream, int64_t live_rows[2]) {
  const char* who = "pxo_train_fwd_bwd_culled";
  PXO_TRY(validate_cfg(cfg));
  PXO_TRY(occ_validate(occ, who));
  PXO_TRY(require_train_precision(cfg, who));
  PXO_TRY(refuse_noise(cfg, randomized, who));
  if (live_rows) live_rows[0] = live_rows[1] = 0;
  return train_fwd_bwd_impl(cfg, params, packed_fwd0, packed_bwd0, packed_fwd1, packed_bwd1, origins, directions, viewdirs,
                            pixels, B, randomized, t_rand, u, sp_points, seed, grads, stats, ws, ws_bytes, grads0_ready, stream,
                            nullptr, nullptr, occ, live_rows, who);
}

int pxo_sg_lobes(const float* sg_params, int K, float* lobes, void* stream) {
  PXO_REQUIRE(sg_params != nullptr, "pxo_sg_lobes: null sg_params ([3K]: sg_lambda [K], then sg_mu_spher [K,2])");
  PXO_REQUIRE(lobes != nullptr, "pxo_sg_lobes: null lobes ([K,4])");
  PXO_REQUIRE(K >= 1 && K <= 25, "pxo_sg_lobes: K %d not in [1,25]", K);
  return launch_sg_lobes(sg_params, K, lobes, (hipStream_t)stream);
}

int pxo_sg_shade_composite_train(const PxoCfg* cfg, const float* lobes, const float* raw_rgb, const float* raw_sigma,
                                 const float* z_vals, const float* directions, const float* viewdirs, const float* pixels,
                                 int64_t B, int S, float* comp_rgb, float* weights, float* ray_sse, float* d_raw_rgb,
                                 float* d_raw_sigma, int64_t n_sp, float* sp_exp, float* d_lobes, float* lobe_partials,
                                 void* stream) {
  PXO_TRY(validate_cfg(cfg));
  const int K = sh_dim(cfg->sh_deg);
  PXO_REQUIRE(lobes != nullptr, "pxo_sg_shade_composite_train: null lobes ([sg_dim,4] with sg_dim = (sh_deg+1)^2 = %d)", K);
  PXO_REQUIRE(d_lobes != nullptr && lobe_partials != nullptr,
              "pxo_sg_shade_composite_train: null d_lobes ([%d,4]) or lobe_partials (%d floats per %d rays)", K, 4 * K,
              PXO_SG_RAYS_PER_BLOCK);
  PXO_REQUIRE(B >= 0 && n_sp >= 0, "pxo_sg_shade_composite_train: bad sizes B=%lld n_sp=%lld", (long long)B, (long long)n_sp);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return launch_fill(d_lobes, 4 * K, 0.f, s);
  PXO_REQUIRE(raw_rgb && raw_sigma && z_vals && directions && viewdirs && pixels && ray_sse && d_raw_rgb && d_raw_sigma &&
                  (n_sp == 0 || sp_exp),
              "pxo_sg_shade_composite_train: bad arguments");
  PXO_TRY(launch_shade_composite_train(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, pixels, B, S, comp_rgb, weights,
                                       ray_sse, d_raw_rgb, d_raw_sigma, n_sp, sp_exp, lobes, lobe_partials, s));
  return launch_sg_lobe_grad(lobe_partials, sg_ray_blocks(B), nullptr, 0, K, nullptr, 0.f, d_lobes, nullptr, nullptr, s);
}

int pxo_sg_train_fwd_bwd_bucketed(const PxoCfg* cfg, const float* params, const float* sg_params, const float* packed_fwd0,
                                  const float* packed_bwd0, const float* packed_fwd1, const float* packed_bwd1,
                                  const float* origins, const float* directions, const float* viewdirs, const float* pixels,
                                  int64_t B, int randomized, const float* t_rand, const float* u, const float* sp_points,
                                  uint64_t seed, float* grads, float* sg_grads, float* stats, void* ws, size_t ws_bytes,
                                  void* grads0_ready, void* stream) {
  PXO_REQUIRE(sg_params != nullptr, "pxo_sg_train_fwd_bwd: null sg_params ([3K]: sg_lambda [K], then sg_mu_spher [K,2])");
  PXO_REQUIRE(sg_grads != nullptr, "pxo_sg_train_fwd_bwd: null sg_grads ([3K])");
  return train_fwd_bwd_impl(cfg, params, packed_fwd0, packed_bwd0, packed_fwd1, packed_bwd1, origins, directions, viewdirs,
                            pixels, B, randomized, t_rand, u, sp_points, seed, grads, stats, ws, ws_bytes, grads0_ready, stream,
                            sg_params, sg_grads, nullptr, nullptr, "pxo_sg_train_fwd_bwd");
}

int pxo_sg_train_fwd_bwd(const PxoCfg* cfg, const float* params, const float* sg_params, const float* packed_fwd0,
                         const float* packed_bwd0, const float* packed_fwd1, const float* packed_bwd1, const float* origins,
                         const float* directions, const float* viewdirs, const float* pixels, int64_t B, int randomized,
                         const float* t_rand, const float* u, const float* sp_points, uint64_t seed, float* grads,
                         float* sg_grads, float* stats, void* ws, size_t ws_bytes, void* stream) {
  return pxo_sg_train_fwd_bwd_bucketed(cfg, params, sg_params, packed_fwd0, packed_bwd0, packed_fwd1, packed_bwd1, origins,
                                       directions, viewdirs, pixels, B, randomized, t_rand, u, sp_points, seed, grads, sg_grads,
                                       stats, ws, ws_bytes, nullptr, stream);
}

int pxo_train_fwd_bwd(const PxoCfg* cfg, const float* params, const float* packed_fwd0, const float* packed_bwd0,
                      const float* packed_fwd1, const float* packed_bwd1, const float* origins,
                      const float* directions, const float* viewdirs, const float* pixels, int64_t B, int randomized,
                      const float* t_rand, const float* u, const float* sp_points, uint64_t seed, float* grads,
                      float* stats, void* ws, size_t ws_bytes, void* stream) {
  return pxo_train_fwd_bwd_bucketed(cfg, params, packed_fwd0, packed_bwd0, packed_fwd1, packed_bwd1, origins, directions,
                                    viewdirs, pixels, B, randomized, t_rand, u, sp_points, seed, grads, stats, ws, ws_bytes,
                                    nullptr, stream);
}

int pxo_train_backward_work(const PxoCfg* cfg, int64_t B, void* ws, size_t ws_bytes, int64_t* live_chunks,
                            int64_t* total_chunks, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(B >= 1 && ws && live_chunks && total_chunks, "pxo_train_backward_work: bad arguments");
  Layout L;
  PXO_TRY(lay_out(cfg, B, ws, ws_bytes, true, false, false, "pxo_train_backward_work", L));
  const TrainWs& t = L.t;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nc = (t.c.M + kLiveRows - 1) / kLiveRows, nf = cfg->num_fine_samples > 0 ? (t.f.M + kLiveRows - 1) / kLiveRows : 0;
  *total_chunks = nc + nf;
  // dense pass (also when the step fell back to it because a row range would not fit the live lists): every chunk is live.
  // The mode is the one the last step on this workspace RECORDED in it, not one re-derived from today's tuning knobs.
  unsigned int record = 0;
  if (hipMemcpyAsync(&record, t.scalars + kStepWordsAt, sizeof(record), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("pxo_train_backward_work: copy back failed");
    return PXO_ERR_HIP;
  }
  if (record == kStepRecordCulled) {
    set_error("pxo_train_backward_work: the last step on this workspace was pxo_train_fwd_bwd_culled, whose reverse pass ran on the "
              "live rows only (the chunk totals of the dense row count do not describe it; see its live_rows)");
    return PXO_ERR_ARG;
  }
  if ((record & ~1u) != kStepRecord) { set_error("pxo_train_backward_work: no pxo_train_fwd_bwd call has used this workspace"); return PXO_ERR_ARG; }
  if (!(record & 1u)) {
    *live_chunks = nc + nf;
    return PXO_OK;
  }
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(t.scalars + 96);     // 8-byte aligned tail of the scalars block
  if (hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s) != hipSuccess) { set_error("hipMemsetAsync failed"); return PXO_ERR_HIP; }
  PXO_TRY(launch_count_live(t.c.live, nc, cnt, s));
  if (nf > 0) PXO_TRY(launch_count_live(t.f.live, nf, cnt, s));
  unsigned long long host = 0;
  if (hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("pxo_train_backward_work: copy back failed");
    return PXO_ERR_HIP;
  }
  *live_chunks = (int64_t)host;
  return PXO_OK;
}

// plain handles for the bucketed form: the caller's runtime (torch) creates its events lazily and keeps them private
int pxo_event_create(void** event) {
  PXO_REQUIRE(event != nullptr, "pxo_event_create: NULL pointer");
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreateWithFlags failed"); return PXO_ERR_HIP; }
  *event = (void*)e;
  return PXO_OK;
}
int pxo_event_destroy(void* event) {
  if (event && hipEventDestroy((hipEvent_t)event) != hipSuccess) { set_error("hipEventDestroy failed"); return PXO_ERR_HIP; }
  return PXO_OK;
}
int pxo_stream_wait_event(void* stream, void* event) {
  PXO_REQUIRE(event != nullptr, "pxo_stream_wait_event: NULL event");
  if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); return PXO_ERR_HIP; }
  return PXO_OK;
}

int pxo_adam_pack_step(const PxoCfg* cfg, float* params, float* m, float* v, const float* grads, float lr, int64_t step,
                       float grad_scale, float* packed_fwd0, float* packed_bwd0, float* packed_fwd1, float* packed_bwd1,
                       void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(params && m && v && grads && step >= 0 && packed_fwd0 && packed_fwd1, "pxo_adam_pack_step: bad arguments");
  PXO_REQUIRE((packed_bwd0 != nullptr) == (packed_bwd1 != nullptr), "pxo_adam_pack_step: both backward images or none");
  if (cfg->mlp_precision != PXO_MLP_F32) {
    // split-precision images: the Adam kernel, then that precision's packing kernels (same results as the separate calls)
    if (cfg->mlp_precision == PXO_MLP_BF16X3 && packed_bwd0) {
      set_error("pxo_adam_pack_step: the bf16x3 images are forward-only (packed_bwd must be NULL)");
      return PXO_ERR_UNSUPPORTED;
    }
    const int64_t n_mlp = mlp_param_count(cfg->sh_deg);
    PXO_TRY(launch_adam(params, m, v, grads, 2 * n_mlp, lr, step, grad_scale, (hipStream_t)stream));
    PXO_TRY(launch_pack(cfg, params, packed_fwd0, packed_bwd0, (hipStream_t)stream));
    return launch_pack(cfg, params + n_mlp, packed_fwd1, packed_bwd1, (hipStream_t)stream);
  }
  return launch_adam_pack(cfg, params, m, v, grads, lr, step, grad_scale, packed_fwd0, packed_bwd0, packed_fwd1,
                          packed_bwd1, (hipStream_t)stream);
}

int pxo_occupy_cus(int blocks, int threads, float micros, int lds_bytes, void* stream) {
  PXO_REQUIRE(blocks >= 1 && blocks <= 4096 && threads >= 64 && threads <= 1024 && threads % 64 == 0 && micros >= 0.f &&
                  micros <= 1e6f && lds_bytes >= 0 && lds_bytes <= 65536,
              "pxo_occupy_cus: bad arguments (blocks %d, threads %d, micros %g, lds_bytes %d)", blocks, threads, (double)micros,
              lds_bytes);
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
    khz = 100000;                                                    // gfx9: 100 MHz constant clock
  const long long ticks = (long long)((double)micros * 1e-3 * (double)khz);
  hipLaunchKernelGGL(occupy_kernel, dim3(blocks), dim3(threads), (size_t)lds_bytes, (hipStream_t)stream, ticks);
  return check_launch("occupy_cus");
}

int pxo_profile_enable(int tag_mask) {
  PXO_REQUIRE(tag_mask >= 0 && tag_mask < (1 << PXO_PROF_NUM_TAGS), "pxo_profile_enable: mask %d has bits beyond the %d tags",
              tag_mask, PXO_PROF_NUM_TAGS);
  g_prof_mask = (unsigned)tag_mask;
  return PXO_OK;
}

int pxo_profile_read(int tag, int64_t* launches, double* total_ms, int64_t* total_rows) {
  PXO_REQUIRE(tag >= 0 && tag < PXO_PROF_NUM_TAGS && launches && total_ms && total_rows, "pxo_profile_read: bad arguments");
  int64_t n = 0, rows = 0;
  double ms = 0.0;
  std::vector<ProfRecord> keep;
  for (auto& r : g_prof) {
    if (r.tag != tag) { keep.push_back(r); continue; }
    float t = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
      ++n; ms += t; rows += r.rows;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof.swap(keep);
  *launches = n; *total_ms = ms; *total_rows = rows;
  return PXO_OK;
}

int pxo_eval_points(const PxoCfg* cfg, const float* packed_fwd, const float* points, int64_t N, float* raw_rgb,
                    float* raw_sigma, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  if (N == 0) return PXO_OK;
  PXO_REQUIRE(N >= 0 && packed_fwd && points && raw_sigma, "pxo_eval_points: bad arguments");
  return launch_mlp_fwd(cfg, packed_fwd, points, N, raw_rgb, raw_sigma, nullptr, nullptr, nullptr,
                        (hipStream_t)stream);
}

int pxo_grid_sigma(const PxoCfg* cfg, const float* packed_fwd, int reso, int x0, int x1, const float offset[3],
                   const float scale[3], float* sigma_out, void* stream) {
  PXO_TRY(validate_cfg(cfg));
  PXO_REQUIRE(reso >= 1 && x0 >= 0 && x1 >= x0 && x1 <= reso, "pxo_grid_sigma: bad slab [%d,%d) of %d", x0, x1, reso);
  if (x1 == x0) return PXO_OK;
  PXO_REQUIRE(packed_fwd && offset && scale && sigma_out, "pxo_grid_sigma: NULL pointer");
  return launch_mlp_fwd_grid(cfg, packed_fwd, reso, x0, x1, offset, scale, sigma_out, (hipStream_t)stream);
}

}  // extern "C"
