// api.hip -- extern "C" entry points of liblograst.so (declared in include/lograst.h), launch
// sequencing, error text and the HIP-event per-kernel timer.  No allocation, no host sync except where
// the header says so.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <atomic>
#include <string>
#include <vector>

#include "common.hpp"
#include "launch.hpp"
#include "decide.hpp"

static thread_local std::string g_err;
static int lr_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define LR_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return lr_fail(LOGRAST_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));              \
  } while (0)

static int lr_env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? std::atoi(e) : dflt;
}
// ---- performance knobs ------------------------------------------------------------------------------------
// The one table (common.hpp: LrKnob): name = the environment variable, default, range, what lograst_knob_info tells log_amd.tune.
struct LrKnobInfo { LrKnob id; const char* name; int dflt, lo, hi; const char* what; };
static constexpr LrKnobInfo kKnobs[] = {
    {LRKNOB_HELPER_MIN_N, "LOGRAST_HELPER_MIN_N", 4000000, 0, 2000000000, "Gaussians from which the helper passes (absolute slot table, touched-only dL/dconic clearing, separate zero-fill kernels) pay for their launches"},
    {LRKNOB_HIT_MASKS, "LOGRAST_HIT_MASKS", 1, 0, 2, "the compositing kernels leave their per-chunk hit masks in lograst_view.hit_masks (when the caller provides it) and the reverse walk reads them instead of running the support tests again: 1 = row-split form records the entries some pixel of the 4x4 block accumulated (quadrant form: the support ballots), 2 = the support ballots in both forms (a superset: same gradients, more visits); 0 = ignore the buffer"},
    {LRKNOB_LAZY_SORT, "LOGRAST_LAZY_SORT", 1, 0, 1, "lists of more than 4096 keys are ordered over their first window (7680 positions) only; tiles whose walk needs more are marked by the compositing kernels and finished by a second, normally idle sort + compositing pair; 0 = every list to its end up front"},
    {LRKNOB_PBWD_LIST, "LOGRAST_PBWD_LIST", 1, 0, 2, "large inputs with running-sum gradients: the chain rule runs over a compact list of the rows with point_weight > 0 (a streaming compaction pass + a list pass) instead of one kernel that tests every row: 0 never, 1 on band views, 2 always"},
    {LRKNOB_MID_RANK, "LOGRAST_MID_RANK", 1, 0, 1, "rects of 5..16 tiles are RANKED by the batched projection (LDS atomics; 32-byte rank rows in geom), so the fill places them without cursor atomics or support tests; 0 = counted only, placed through the per-tile cursors"},
    {LRKNOB_MID_COOP, "LOGRAST_MID_COOP", 16, 0, 64, "rects of 5..16 tiles are counted (projection: in waves that hold at most this many of them) and placed (fill: any non-zero value) by the whole wave, four rects per pass, instead of by their lane; 0 = per lane"},
    {LRKNOB_DEFER_TILES, "LOGRAST_DEFER_TILES", LR_COOP_TILES, 4, 4096, "rects above this many tiles are counted by lr_count_huge_kernel (one wave per rect) instead of by their lane"},
    {LRKNOB_HUGE_CHUNK, "LOGRAST_HUGE_CHUNK", LR_HUGE_CHUNK, 256, 8192, "Gaussians per workgroup of lr_count_huge_kernel (multiple of 256)"},
    {LRKNOB_BATCH_PLANES, "LOGRAST_BATCH_PLANES", 4, 1, 4, "consecutive projection batches one workgroup owns"},
    {LRKNOB_BATCH_SLOTS, "LOGRAST_BATCH_SLOTS", 256, 64, 1024, "workgroups per round the batched projection sizes its batches for"},
    {LRKNOB_SEPARATE_ZERO, "LOGRAST_SEPARATE_ZERO", 1, 0, 1, "large inputs: zero-fills streamed by kernels of their own instead of inside the fill kernel"},
    {LRKNOB_FILL_XCD_ORDER, "LOGRAST_FILL_XCD_ORDER", 1, 0, 1, "fill kernel walks the Gaussians XCD-contiguously"},
    {LRKNOB_FILL_NT, "LOGRAST_FILL_NT", 1, 0, 1, "fill kernel: non-temporal streams for the fill records and zero-fills"},
    {LRKNOB_XCD_MODE, "LOGRAST_XCD_MODE", 3, 0, 3, "blockIdx -> tile mapping of the compositing kernels (3 = longest list first)"},
    {LRKNOB_PROJECT_BLOCKS, "LOGRAST_PROJECT_BLOCKS", 512, 64, 65536, "grid cap of the unbatched projection kernel"},
    {LRKNOB_BWD_ROWS, "LOGRAST_BWD_ROWS", 2, 0, 2, "reverse walk: 1 = row-split form (four 4x4 blocks per wave), 0 = one quadrant per wave, 2 = the view's walk_form hint (none: row-split from LOGRAST_HELPER_MIN_N Gaussians)"},
    {LRKNOB_FWD_ROWS, "LOGRAST_FWD_ROWS", 2, 0, 2, "compositing: 1 = row-split form (four 4x4 blocks per wave), 0 = one quadrant per wave, 2 = the view's walk_form hint"},
    {LRKNOB_FILL_STAGED, "LOGRAST_FILL_STAGED", 2, 0, 3, "bucket fill of batched full views: K = the batch's slot-table row staged in LDS by workgroups of up to K x 1024 consecutive Gaussians (K per thread), 0 = one table look-up per tile instance"},
    {LRKNOB_FILL_PER_THREAD, "LOGRAST_FILL_PER_THREAD", 1, 1, 4, "bucket fill: Gaussians per thread (their fill records are requested together): 1, 2 or 4"},
    {LRKNOB_BAND_SPARSE, "LOGRAST_BAND_SPARSE", 1, 0, 1, "band views (tile_row_begin/end a proper part of the grid): 1 = the band projection (Gaussians without a rect cost 44 bytes, survivors compacted into full waves), 0 = the full-view kernel"},
    {LRKNOB_FWD_BLOCK_TEST, "LOGRAST_FWD_BLOCK_TEST", 1, 0, 1, "row-split compositing: 1 = exact support test per 4x4 block, 0 = exact for the quadrant + bounding box per block (the reverse walk on the forward's hit masks visits what the forward's test kept)"},
    {LRKNOB_BWD_BLOCK_TEST, "LOGRAST_BWD_BLOCK_TEST", 1, 0, 1, "row-split reverse walk: 1 = exact support test per 4x4 block, 0 = exact for the quadrant + bounding box per block"},
};
static constexpr bool lr_knobs_in_enum_order() {
  for (int i = 0; i < LRKNOB_COUNT; i++)
    if (kKnobs[i].id != i) return false;
  return true;
}
static_assert(sizeof(kKnobs) / sizeof(kKnobs[0]) == LRKNOB_COUNT && lr_knobs_in_enum_order(), "kKnobs[]: one row per LrKnob, in the enum's order");
static std::mutex g_knob_mu;
static bool g_knob_set[LRKNOB_COUNT];            // lograst_set_knob overrides (under g_knob_mu)
static int32_t g_knob_over[LRKNOB_COUNT];
static std::atomic<int32_t> g_knob_val[LRKNOB_COUNT];   // what the next launch reads
static std::atomic<bool> g_knobs_resolved{false};
static void lr_resolve_knobs_locked() {
  for (int i = 0; i < LRKNOB_COUNT; i++)
    g_knob_val[i].store(g_knob_set[i] ? g_knob_over[i] : lr_env_int(kKnobs[i].name, kKnobs[i].dflt), std::memory_order_relaxed);
  g_knobs_resolved.store(true, std::memory_order_release);
}
int lr_knob(LrKnob k) {
  if (!g_knobs_resolved.load(std::memory_order_acquire)) {   // first use in this process
    std::lock_guard<std::mutex> lk(g_knob_mu);
    if (!g_knobs_resolved.load(std::memory_order_relaxed)) lr_resolve_knobs_locked();
  }
  return g_knob_val[k].load(std::memory_order_relaxed);
}

// ---- the plan of a forward ----------------------------------------------------------------------------------
// Every launch decision of a forward that depends on (view, n) only, made once per entry point (lr_plan) and handed to both
// stages: stage 1 skips lr_rebase_kernel exactly when stage 2's fill stages the slot-table row, because both read `staged_k`.
struct LrPlan {
  uint32_t tiles;
  uint32_t batch, planes;   // Gaussians per projection batch (0 = unbatched kernel), consecutive batches per workgroup
  uint32_t batches;
  bool band;                // the batched projection runs in its band form (project.hip: lr_band_sparse)
  int staged_k;             // the fill stages the batch's slot-table row in LDS, K Gaussians per thread (0 = look-up form)
  bool big_input;           // n >= LOGRAST_HELPER_MIN_N: the helper passes pay for their launches
};
// Gaussians per projection batch (project.hip: lr_project_batched_kernel), 0 = unbatched kernel, and the number of
// consecutive batches one workgroup owns (`planes`: one plane of LDS tile counters each).  A batch is big enough that it
// puts several instances into a tile (that is what it saves in memory-side atomics) and at most 32768 Gaussians (16-bit
// ranks); a workgroup takes as many batches as its LDS holds (up to 4), which makes the runs it reserves in a tile
// adjacent (longer contiguous key writes in the fill) and leaves one workgroup per CU per round.
// LOGRAST_BATCH_PLANES caps the planes.
static void lr_pick_batch(LrPlan& p, int32_t n, uint32_t gx, uint32_t gy) {
  const uint32_t tiles = p.tiles, max_planes = (uint32_t)lr_knob(LRKNOB_BATCH_PLANES);
  p.batch = 0u; p.planes = 1u;
  if (n <= 0 || tiles > LR_BATCH_MAX_TILES || gx > 8191u || gy > 8191u) return;  // 13-bit tile coordinates in the fill record
  uint32_t smax = (uint32_t)(LR_BATCH_LDS_BYTES / (sizeof(uint32_t) * (size_t)tiles));
  if (smax > max_planes) smax = max_planes;
  if (smax > 4u) smax = 4u;
  if (smax < 1u) smax = 1u;
  // One workgroup of 1024 threads per CU (82 VGPRs): 256 run at a time.  Size the work so that the workgroups fill
  // whole rounds of 256 (10 M Gaussians: 306 batches of 32768 = 1.2 rounds ran as long as 2).
  const int slots_k = lr_knob(LRKNOB_BATCH_SLOTS);
  const uint32_t slots = (uint32_t)(slots_k > 0 ? slots_k : kKnobs[LRKNOB_BATCH_SLOTS].dflt);
  const uint64_t per_round = (uint64_t)slots * 32768u * smax;
  const uint32_t rounds = (uint32_t)(((uint64_t)n + per_round - 1u) / per_round);
  const uint32_t groups = slots * rounds;                                  // workgroups
  const uint32_t g = ((uint32_t)n + groups - 1u) / groups;                 // Gaussians per workgroup
  uint32_t planes = (g + 32767u) / 32768u;
  if (planes < 1u) planes = 1u;
  if (planes > smax) planes = smax;
  uint32_t b = ((g + planes - 1u) / planes + 2047u) / 2048u * 2048u;   // (multiples of 2048: a fill workgroup of 1024 threads x 2 stays inside one batch)
  if (b < 4096u) b = 4096u;
  if (b > 32768u) b = 32768u;
  p.batch = b; p.planes = planes;
}
// Does the fill of this view stage the batch's slot-table row in LDS (project.hip: lr_fill_staged_kernel), and with how
// many Gaussians per thread?  0 = no (unbatched, band form, tile grids whose row does not fit: the look-up form).  K x 1024
// consecutive Gaussians of a workgroup share one table row: the largest K <= the knob that divides the batch.
static int lr_fill_staged_k(const LrPlan& p) {
  const int staged_knob = lr_knob(LRKNOB_FILL_STAGED);
  if (staged_knob <= 0 || p.batch == 0u || p.tiles > LR_FILL_STAGED_MAX_TILES || p.band) return 0;
  if (p.batch % LR_FILL_STAGED_ROWS != 0u) return 0;
  const int per_batch = (int)(p.batch / LR_FILL_STAGED_ROWS);
  int K = staged_knob > 3 ? 3 : staged_knob;
  while (K > 1 && per_batch % K != 0) K--;
  return K;
}
// The helper passes pay for their launch only on large inputs (each is ~10 us at 1 M Gaussians, where the work they
// save is smaller than that): lr_rebase_kernel (absolute slot table for the fill), the touched-only clearing of
// dL/dconic, the separate zero-fill kernels, and in the backward the row-split reverse walk and the chain rule's
// streamed dL/dmeans2D zeros.
static bool lr_big_input(int32_t n) { return n >= lr_knob(LRKNOB_HELPER_MIN_N); }
static LrPlan lr_plan(const LrView& v, int32_t n) {
  LrPlan p;
  p.tiles = (uint32_t)v.gx * (uint32_t)v.gy;
  lr_pick_batch(p, n, (uint32_t)v.gx, (uint32_t)v.gy);
  p.batches = p.batch ? ((uint32_t)n + p.batch - 1u) / p.batch : 0u;
  p.band = lr_band_sparse(v, (int)p.batch);
  p.staged_k = lr_fill_staged_k(p);
  p.big_input = lr_big_input(n);
  return p;
}

// Support cull in the binning kernels (project.hip): on unless LOGRAST_TILE_CULL=0 or lograst_set_tile_cull(0).
static std::atomic<int> g_tile_cull{-1};
static int lr_tile_cull() {
  int c = g_tile_cull.load(std::memory_order_relaxed);
  if (c < 0) {
    c = lr_env_int("LOGRAST_TILE_CULL", 1) ? 1 : 0;
    g_tile_cull.store(c, std::memory_order_relaxed);
  }
  return c;
}

// ---- profiling ------------------------------------------------------------------------------------------
static const char* kKernelNames[LOGRAST_NUM_KERNELS] = {
    "compute_radius", "project", "scan_tiles", "fill_keys", "sort_small", "sort_large", "sort_huge",
    "blend_fwd", "blend_bwd", "project_bwd", "knn3", "lod_traverse", "counter_update", "sparse_adam",
    "id_histogram", "gather_activate", "activate_bwd", "count_huge", "rebase_slots", "lazy_tail",
    "loss_fwd", "loss_bwd", "recolor"};
struct ProfRec { int slot; hipEvent_t a, b; bool own_a; };
// Consecutive launches inside one entry point share an event: the end of kernel k is the begin of kernel k+1 (N+1
// events for a chain of N kernels instead of 2N; every recorded event costs ~1.4 us of stream time).
struct ProfLast { hipStream_t stream; unsigned long long call; hipEvent_t ev; bool valid; };
static thread_local unsigned long long g_prof_call = 0;   // bumped at every entry point that launches kernels
static ProfLast g_prof_last = {nullptr, 0, nullptr, false};
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof_open;     // begin recorded, waiting for end
static std::vector<ProfRec> g_prof_done;
static std::vector<hipEvent_t> g_event_pool;
static double g_prof_ms[LOGRAST_NUM_KERNELS];
static int64_t g_prof_cnt[LOGRAST_NUM_KERNELS];
static std::mutex g_prof_mu;

static hipEvent_t lr_get_event() {
  if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void lr_prof_begin(int slot, hipStream_t s) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r{slot, nullptr, lr_get_event(), true};
  if (g_prof_last.valid && g_prof_last.stream == s && g_prof_last.call == g_prof_call) {
    r.a = g_prof_last.ev;   // nothing was enqueued on s since that event: it marks this kernel's begin too
    r.own_a = false;
  } else {
    r.a = lr_get_event();
    (void)hipEventRecord(r.a, s);
  }
  g_prof_last.valid = false;
  g_prof_open.push_back(r);
}
void lr_prof_end(int slot, hipStream_t s) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (size_t i = g_prof_open.size(); i-- > 0;) {
    if (g_prof_open[i].slot == slot) {
      (void)hipEventRecord(g_prof_open[i].b, s);
      g_prof_last = ProfLast{s, g_prof_call, g_prof_open[i].b, true};
      g_prof_done.push_back(g_prof_open[i]);
      g_prof_open.erase(g_prof_open.begin() + (long)i);
      return;
    }
  }
}
static void lr_prof_drain_locked() {
  for (auto& r : g_prof_done) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      g_prof_ms[r.slot] += ms;
      g_prof_cnt[r.slot] += 1;
    }
    if (r.own_a) g_event_pool.push_back(r.a);
    g_event_pool.push_back(r.b);
  }
  g_prof_done.clear();
}

static int lr_make_view(const lograst_view* in, LrView* out) {
  if (!in) return lr_fail(LOGRAST_ERR_ARG, "view is NULL");
  if (in->width <= 0 || in->height <= 0) return lr_fail(LOGRAST_ERR_ARG, "image size must be positive");
  if (in->width > 65535 * 16 || in->height > 65535 * 16 ||
      (size_t)((in->width + 15) / 16) * (size_t)((in->height + 15) / 16) > 131072)
    return lr_fail(LOGRAST_ERR_ARG, "image too large (more than 131072 tiles)");
  if (!in->viewmatrix || !in->projmatrix || !in->bg) return lr_fail(LOGRAST_ERR_ARG, "viewmatrix/projmatrix/bg must be device pointers");
  if (in->filter_mode < 0 || in->filter_mode > 2) return lr_fail(LOGRAST_ERR_ARG, "bad filter_mode");
  out->W = in->width; out->H = in->height;
  out->gx = (in->width + LOGRAST_TILE - 1) / LOGRAST_TILE;
  out->gy = (in->height + LOGRAST_TILE - 1) / LOGRAST_TILE;
  out->ty0 = 0; out->ty1 = out->gy;
  if (in->tile_row_begin != 0 || in->tile_row_end != 0) {
    if (in->tile_row_begin < 0 || in->tile_row_end <= in->tile_row_begin || in->tile_row_end > out->gy)
      return lr_fail(LOGRAST_ERR_ARG, "tile_row_begin / tile_row_end outside the tile grid");
    out->ty0 = in->tile_row_begin; out->ty1 = in->tile_row_end;
  }
  out->tanfovx = in->tanfovx; out->tanfovy = in->tanfovy;
  out->fx = (float)in->width / (2.0f * in->tanfovx);
  out->fy = (float)in->height / (2.0f * in->tanfovy);
  out->scale_modifier = in->scale_modifier;
  out->filter_mode = in->filter_mode; out->ndc_cull = in->ndc_cull; out->extras = in->extras;
  out->view = in->viewmatrix; out->proj = in->projmatrix; out->bg = in->bg;
  out->cov3d = in->cov3d_precomp; out->g_cov3d = in->dl_dcov3d;
  if (in->walk_form < LOGRAST_FORM_AUTO || in->walk_form > LOGRAST_FORM_QUADRANT) return lr_fail(LOGRAST_ERR_ARG, "bad walk_form");
  out->walk_form = in->walk_form;
  if (in->hit_masks && (reinterpret_cast<uintptr_t>(in->hit_masks) & 31u)) return lr_fail(LOGRAST_ERR_ARG, "hit_masks must be 32-byte aligned");
  out->masks = lr_knob(LRKNOB_HIT_MASKS) ? in->hit_masks : nullptr;
  out->mask_words = in->hit_mask_words;
  if (in->hit_mask_form < 0 || in->hit_mask_form > 2) return lr_fail(LOGRAST_ERR_ARG, "bad hit_mask_form");
  out->mask_form = in->hit_mask_form;
  return LOGRAST_OK;
}

extern "C" {

int lograst_version(void) { return LOGRAST_VERSION; }
const char* lograst_last_error(void) { return g_err.c_str(); }

size_t lograst_tile_state_bytes(int32_t width, int32_t height, int32_t n) {
  LrView v = {};   // the whole image: the tile grid is all of a view that the batching looks at
  v.W = width; v.H = height;
  v.gx = (int)((uint32_t)(width + LOGRAST_TILE - 1) / LOGRAST_TILE); v.gy = (int)((uint32_t)(height + LOGRAST_TILE - 1) / LOGRAST_TILE);
  v.ty1 = v.gy;
  const LrPlan p = lr_plan(v, n);
  return sizeof(uint32_t) * lr_state_words(p.tiles, p.batches);
}
size_t lograst_geom_bytes(int32_t n) {  // 64-byte records + the 16-byte fill records of the batched projection + a 4-byte index each (band views) + the rank rows of the 5..16-tile rects (common.hpp)
  const size_t nn = (size_t)(n > 0 ? n : 0);
  return lr_midrank_off_bytes(nn) + lr_midrank_bytes(nn);
}
size_t lograst_record_bytes(int32_t n) { return sizeof(float) * LOGRAST_REC_FLOATS * (size_t)(n > 0 ? n : 0); }   // the records alone: all of geom that the compositing kernels and the reverse walk read
size_t lograst_keys_bytes(uint32_t capacity) { return 2 * sizeof(uint64_t) * (size_t)capacity; }  // keys + sort scratch
int lograst_forward_form(const lograst_view* view) {
  LrView v;
  int rc = lr_make_view(view, &v);
  if (rc) return rc;
  return lr_blend_fwd_form(v);
}
int lograst_backward_form(const lograst_view* view, int32_t n) {
  LrView v;
  int rc = lr_make_view(view, &v);
  if (rc) return rc;
  return lr_blend_bwd_form(v, lr_big_input(n));
}
size_t lograst_hit_mask_bytes(uint32_t capacity, int32_t width, int32_t height) {   // blend.hip: 16 words per (tile, 64-entry chunk) slot
  const size_t gx = (size_t)(width > 0 ? (width + LOGRAST_TILE - 1) / LOGRAST_TILE : 0), gy = (size_t)(height > 0 ? (height + LOGRAST_TILE - 1) / LOGRAST_TILE : 0);
  return 16 * sizeof(uint64_t) * ((size_t)capacity / 64 + gx * gy + 1);
}
size_t lograst_list_bytes(uint32_t capacity) { return sizeof(uint32_t) * (size_t)capacity; }

const uint32_t* lograst_tile_offsets(const void* tile_state, int32_t width, int32_t height) {
  uint32_t gx = (uint32_t)(width + LOGRAST_TILE - 1) / LOGRAST_TILE, gy = (uint32_t)(height + LOGRAST_TILE - 1) / LOGRAST_TILE;
  return reinterpret_cast<const uint32_t*>(tile_state) + lr_offsets_off(gx * gy);
}

// Lazily ordered lists (LOGRAST_LAZY_SORT; common.hpp: sorted[]): how much of every tile's list is in final order, and
// the call that orders the rest -- for callers that want the complete lists (the parity tests do).
int lograst_ordered_lengths(const void* tile_state, int32_t width, int32_t height, uint32_t* lengths_out, void* stream) {
  g_prof_call++;
  if (!tile_state || !lengths_out) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (width <= 0 || height <= 0) return lr_fail(LOGRAST_ERR_ARG, "bad image size");
  const uint32_t gx = (uint32_t)(width + LOGRAST_TILE - 1) / LOGRAST_TILE, gy = (uint32_t)(height + LOGRAST_TILE - 1) / LOGRAST_TILE;
  lr_launch_ordered_lengths(reinterpret_cast<const uint32_t*>(tile_state), gx * gy, lengths_out, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_finish_lists(void* tile_state, int32_t width, int32_t height, void* keys, uint32_t* point_list,
                         uint32_t capacity, void* stream) {
  g_prof_call++;
  if (!tile_state) return lr_fail(LOGRAST_ERR_ARG, "tile_state is NULL");
  if (width <= 0 || height <= 0) return lr_fail(LOGRAST_ERR_ARG, "bad image size");
  if (capacity == 0) return LOGRAST_OK;
  if (!keys || !point_list) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  const uint32_t gx = (uint32_t)(width + LOGRAST_TILE - 1) / LOGRAST_TILE, gy = (uint32_t)(height + LOGRAST_TILE - 1) / LOGRAST_TILE;
  // The forward documents `keys` as dead after the call; what this entry point orders from must be the very buffer that
  // forward's fill wrote (round-5 advisory: a stale or reused buffer silently corrupted point_list and marked it ordered).
  // The fill left (pointer, capacity) in the header; this diagnostic call reads them back (it synchronises `stream`).
  uint32_t hdr[LR_HDR_WORDS];
  LR_HIP(hipMemcpyAsync(hdr, tile_state, sizeof(hdr), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  const uint64_t kp = (uint64_t)reinterpret_cast<uintptr_t>(keys);
  if (hdr[LR_HDR_KEYS_LO] != (uint32_t)kp || hdr[LR_HDR_KEYS_HI] != (uint32_t)(kp >> 32) || hdr[LR_HDR_KEYS_CAP] != capacity)
    return lr_fail(LOGRAST_ERR_ARG, "keys / capacity are not the buffer this tile_state's forward filled");
  lr_launch_sort_rest(reinterpret_cast<uint32_t*>(tile_state), gx * gy, reinterpret_cast<uint64_t*>(keys), point_list,
                      capacity, 0, 3, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

int lograst_compute_radius(int32_t p, const float* means3d, const float* scales, const float* rotations,
                           const float* projmatrix, const float* viewmatrix, float focal_x, float focal_y,
                           float tanfovx, float tanfovy, float* radii_out, void* stream) {
  g_prof_call++;
  if (p < 0) return lr_fail(LOGRAST_ERR_ARG, "negative point count");
  if (p == 0) return LOGRAST_OK;
  if (!means3d || !scales || !rotations || !projmatrix || !viewmatrix || !radii_out)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  lr_launch_radius(p, means3d, scales, rotations, projmatrix, viewmatrix, focal_x, focal_y, tanfovx, tanfovy,
                   radii_out, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

// What the four forward entry points share: the parameters of lograst_forward (include/lograst.h), in its order, so that an
// entry point fills it with one braced list, and the two hooks that are lograst_forward_speculative's alone.
struct LrForwardArgs {
  const lograst_view* view; int32_t n;
  const float *means3d, *scales, *rotations, *opacities, *colors; int32_t* radii; void* geom; void* tile_state;   // stage 1
  uint64_t* keys; uint32_t* point_list; uint32_t capacity, max_tile_len;                                           // stage 2
  float *image, *final_t; int32_t* n_contrib; int32_t* point_id_pixel; float *point_weight_pixel, *point_weight;
  float* bwd_scratch; int32_t bwd_scratch_floats; uint32_t* status;
  void* stream;
  int speculative;              // stage 2 is enqueued before the host knows whether `capacity` suffices
  hipEvent_t after_stage1;      // recorded between the stages (or nullptr)
  int aux;                      // the *_aux entry points: aux_colors [n, 3] are composited into aux_image [3, H, W] by the same walk
  const float* aux_colors; float* aux_image;
};

// stage 1 launches: memset of header + counters, projection (+ counting / ranking), tile scan
static void lr_stage1(const LrView& v, const LrPlan& p, const LrForwardArgs& a, uint32_t* st, hipStream_t s) {
  const uint32_t tiles = p.tiles;
  // Counters: batched projection -> dense (ranked[tiles] | big[tiles] right behind the header), unbatched -> one
  // counter per 64 B.  Header and counters are zeroed by ONE memset (offsets/cursors are fully rewritten by the scan).
  const uint32_t cs = p.batch ? 1u : (uint32_t)LR_CTR_STRIDE;
  const uint32_t big_off = p.batch ? lr_ranked_off(tiles) + tiles : lr_big_off(tiles);
  lr_launch_zero_words(st, ((size_t)(big_off + tiles * cs) + 3) & ~(size_t)3, s);   // the words behind the counters (offsets[]) are rewritten by the scan
  lr_launch_project(v, a.n, a.means3d, a.scales, a.rotations, a.opacities, a.colors, a.radii, a.geom, st + lr_ranked_off(tiles),
                    st + big_off, st, st + lr_basetab_off(tiles), (int)p.batch, (int)p.planes, p.band, lr_tile_cull(), s);
  lr_launch_scan(st, tiles, cs, big_off, s);
  if (p.big_input && p.staged_k == 0)   // (the staged fill adds offsets[] itself); only the band's tiles have slot-table entries
    lr_launch_rebase(st, tiles, p.batches, p.band ? (uint32_t)(v.ty0 * v.gx) : 0u, p.band ? (uint32_t)(v.ty1 * v.gx) : tiles, s);
}

// (a list is streamed -- and may be left at its first window -- only above LR_LONG_LIST keys: with a smaller bound on the
// longest list known to the host the lazy machinery is not launched at all)
static inline bool max_tile_len_allows_streaming(uint32_t max_tile_len, uint32_t capacity) {
  const uint32_t m = (max_tile_len == 0 || max_tile_len > capacity) ? capacity : max_tile_len;
  return m > LR_LONG_LIST;
}

// What a stage 2 and a lograst_recomposite decide alike from (view, plan, arguments): who clears what, and whether the lists
// are walked lazily.
// point_weight (atomicMax target) and the optional backward scratch (one 64-byte accumulator row per Gaussian) are
// cleared by a streaming pass over the Gaussians (the fill kernel; lr_recolor_kernel) -- except, in the 5-tuple flavour on
// large inputs, the scratch: only the rows of Gaussians that contribute to a pixel will ever be read, and the compositing
// kernel clears exactly those when it meets them (a separate pass over point_weight afterwards cost 70 us per 30 M-Gaussian
// view, the stores inside the kernel 30)
// LOGRAST_LAZY_SORT (default 1): lists of more than 4096 keys are ordered over their first window only (7680 positions;
// the walk of a view ends far in front of that: common.hpp, sorted[]); the compositing kernels mark the tiles that needed
// more, and the second pair of launches -- idle in every benched view -- finishes exactly those.  0: every list to its
// end before the first compositing pass (what lograst_finish_lists produces afterwards).
struct LrCompositePlan {
  bool touched_only;    // the compositing kernel clears the accumulator rows it meets; nobody clears the others
  float* zero_n;        // point_weight[n] to clear up front, or nullptr
  float* zero_block;    // accumulator rows to clear up front, or nullptr
  int zero_floats;      // ... floats per Gaussian (0 with nullptr)
  int lazy;
};
static LrCompositePlan lr_composite_plan(const LrView& v, const LrPlan& p, const LrForwardArgs& a) {
  LrCompositePlan c;
  c.touched_only = v.extras && a.bwd_scratch_floats > 0 && p.big_input;
  c.zero_block = (a.bwd_scratch_floats > 0 && !c.touched_only) ? a.bwd_scratch : nullptr;
  c.zero_floats = c.zero_block ? a.bwd_scratch_floats : 0;
  c.zero_n = v.extras ? a.point_weight : nullptr;
  c.lazy = (lr_knob(LRKNOB_LAZY_SORT) && max_tile_len_allows_streaming(a.max_tile_len, a.capacity)) ? 1 : 0;
  return c;
}
// The compositing pass over the records `geom` and, after a lazy one, the pass of the waves that parked.  sort_rest: order
// the tails of the lists they parked in first (a forward: the keys are still there).  Without it (lograst_recomposite) the
// tails must already be in order: the walk of an earlier forward over the same geometry and opacities parked the same waves
// at the same places, and its second pair of launches ordered exactly those lists to their end (sort.hip: sorted[] stays at
// the first window, open[] keeps the bits).
static void lr_composite(const LrView& v, const LrPlan& p, const LrForwardArgs& a, const void* geom, const LrCompositePlan& c,
                         uint32_t* st, bool sort_rest, hipStream_t s) {
  LrBlendFwdArgs b = {};
  b.geom = geom; b.state = st; b.tiles = p.tiles; b.plist = a.point_list; b.capacity = a.capacity;
  b.image = a.image; b.final_T = a.final_t; b.n_contrib = a.n_contrib; b.pid = a.point_id_pixel; b.pwp = a.point_weight_pixel;
  b.pw = a.point_weight; b.zero_conic = c.touched_only ? a.bwd_scratch : nullptr; b.big_input = p.big_input ? 1 : 0;
  b.lazy = c.lazy; b.masks = v.masks; b.aux_colors = a.aux_colors; b.aux_image = a.aux_image;
  lr_launch_blend_fwd(v, b, s);
  if (c.lazy) {
    lr_prof_begin(LRK_LAZY_TAIL, s);
    if (sort_rest) lr_launch_sort_rest(st, p.tiles, a.keys, a.point_list, a.capacity, a.max_tile_len, 2, s);
    b.lazy = 2;   // the pass of the waves that parked
    lr_launch_blend_fwd(v, b, s);
    lr_prof_end(LRK_LAZY_TAIL, s);
  }
}

// stage 2 launches: bucket fill (+ zero-fills), per-tile sort, compositing
static int lr_stage2(const LrView& v, const LrPlan& p, const LrForwardArgs& a, uint32_t* st, hipStream_t s) {
  const int32_t n = a.n;
  if (n == 0 && a.status)   // no fill kernel runs: this forward's entries of the status block
    LR_HIP(hipMemsetAsync(a.status + LOGRAST_STATUS_LAST_INSTANCES, 0, 4 * sizeof(uint32_t), s));
  const LrCompositePlan c = lr_composite_plan(v, p, a);
  float* zero_n = c.zero_n;
  int zero_floats = c.zero_floats;
  if (lr_knob(LRKNOB_SEPARATE_ZERO) && p.big_input) {   // large inputs: streamed by kernels of their own (see lr_zero_floats_kernel); knob 0: always inside the fill kernel
    lr_launch_zero_floats(zero_n, (size_t)n, s);
    if (zero_floats > 0) lr_launch_zero_floats(c.zero_block, (size_t)zero_floats * (size_t)n, s);
    zero_n = nullptr; zero_floats = 0;
  }
  lr_launch_fill(n, v.gx, a.geom, st, p.tiles, a.keys, a.capacity, a.max_tile_len, a.status,
                 zero_n, zero_floats > 0 ? c.zero_block : nullptr, zero_floats,
                 (p.big_input && p.staged_k == 0) ? 1 : 0, a.speculative, p.band ? 1 : 0, p.staged_k, s);
  lr_launch_sort(st, p.tiles, a.keys, a.point_list, a.capacity, a.max_tile_len, c.lazy, s);
  lr_composite(v, p, a, a.geom, c, st, true, s);
  return LOGRAST_OK;
}

static int lr_check_stage1_args(const LrView& v, const LrForwardArgs& a) {
  if (a.n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (!a.tile_state) return lr_fail(LOGRAST_ERR_ARG, "tile_state is NULL");
  if (a.n > 0 && (!a.means3d || !a.opacities || !a.colors || !a.radii || !a.geom))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (a.n > 0 && !v.cov3d && (!a.scales || !a.rotations))
    return lr_fail(LOGRAST_ERR_ARG, "scales / rotations are NULL and the view carries no cov3d_precomp");
  if ((reinterpret_cast<uintptr_t>(a.rotations) | reinterpret_cast<uintptr_t>(a.geom) | reinterpret_cast<uintptr_t>(a.tile_state)) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, "rotations / geom / tile_state must be 16-byte aligned");
  return LOGRAST_OK;
}

// backward: scales + rotations with their gradient outputs, or the view's cov3d_precomp with dl_dcov3d
static int lr_check_cov_args(const LrView& v, const float* scales, const float* rotations, const float* dl_dscales,
                             const float* dl_drotations) {
  if (v.cov3d) {
    if (!v.g_cov3d) return lr_fail(LOGRAST_ERR_ARG, "cov3d_precomp is set but dl_dcov3d is NULL");
    return LOGRAST_OK;
  }
  if (!scales || !rotations || !dl_dscales || !dl_drotations) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  return LOGRAST_OK;
}

// sorts: the call fills and sorts (stage 2: needs `keys`); false: it walks lists that are there (lograst_recomposite)
static int lr_check_stage2_args(const LrView& v, const LrForwardArgs& a, bool sorts = true) {
  if (a.n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (!a.tile_state || !a.image || !a.final_t || !a.n_contrib) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (a.capacity > 0 && ((sorts && !a.keys) || !a.point_list)) return lr_fail(LOGRAST_ERR_ARG, "keys/point_list NULL with capacity > 0");
  if (v.extras && (!a.point_id_pixel || !a.point_weight_pixel || (a.n > 0 && !a.point_weight)))
    return lr_fail(LOGRAST_ERR_ARG, "extras requested but output pointers are NULL");
  if ((a.bwd_scratch_floats != 0 && a.bwd_scratch_floats != LOGRAST_BWD_ROW_FLOATS) ||
      (a.bwd_scratch_floats > 0 && a.n > 0 && !a.bwd_scratch))
    return lr_fail(LOGRAST_ERR_ARG, "bwd_scratch: 0 or LOGRAST_BWD_ROW_FLOATS (16) floats per Gaussian and a non-NULL block");
  if (a.bwd_scratch_floats > 0 && (reinterpret_cast<uintptr_t>(a.bwd_scratch) & 63u))
    return lr_fail(LOGRAST_ERR_ARG, "bwd_scratch must be 64-byte aligned (one accumulator row per line)");
  if (v.masks && (size_t)v.mask_words * sizeof(uint64_t) < lograst_hit_mask_bytes(a.capacity, v.W, v.H))
    return lr_fail(LOGRAST_ERR_ARG, "hit_mask_words is smaller than lograst_hit_mask_bytes(capacity, width, height) / 8");
  return LOGRAST_OK;
}

// What the *_aux entry points ask on top (forward: aux_colors / aux_image; backward: its own list): whole images, scales and
// rotations.  The aux walk exists in the quadrant form only, and the chain rule's aux output not next to cov3d_precomp.
static int lr_check_aux_view(const LrView& v) {
  if (v.ty0 != 0 || v.ty1 != v.gy) return lr_fail(LOGRAST_ERR_ARG, "aux channels render whole images only (tile_row_begin / tile_row_end)");
  if (v.cov3d) return lr_fail(LOGRAST_ERR_ARG, "aux channels have no cov3d_precomp form");
  return LOGRAST_OK;
}
static int lr_check_aux_args(const LrView& v, const LrForwardArgs& a) {
  if (a.n > 0 && (!a.aux_colors || !a.aux_image)) return lr_fail(LOGRAST_ERR_ARG, "aux_colors / aux_image are NULL");
  return lr_check_aux_view(v);
}

// The one forward body behind the four entry points and their _aux forms, in two halves (lograst_forward_speculative has checks of its own
// between them): the view and the argument checks of the stages asked for, stage 1's first; then plan and launches.
static int lr_forward_check(const LrForwardArgs& a, bool stage1, bool stage2, LrView* v) {
  g_prof_call++;
  int rc = lr_make_view(a.view, v);
  if (rc) return rc;
  if (stage1 && (rc = lr_check_stage1_args(*v, a))) return rc;
  if (stage2 && (rc = lr_check_stage2_args(*v, a))) return rc;
  if (a.aux && (rc = lr_check_aux_args(*v, a))) return rc;
  return LOGRAST_OK;
}
static int lr_forward_launch(const LrView& v, const LrForwardArgs& a, bool stage1, bool stage2) {
  int rc;
  const LrPlan p = lr_plan(v, a.n);
  hipStream_t s = (hipStream_t)a.stream;
  uint32_t* st = reinterpret_cast<uint32_t*>(a.tile_state);
  if (stage1) lr_stage1(v, p, a, st, s);
  if (a.after_stage1) LR_HIP(hipEventRecord(a.after_stage1, s));
  if (stage2 && (rc = lr_stage2(v, p, a, st, s))) return rc;
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
static int lr_forward(const LrForwardArgs& a, bool stage1, bool stage2) {
  LrView v;
  const int rc = lr_forward_check(a, stage1, stage2, &v);
  return rc ? rc : lr_forward_launch(v, a, stage1, stage2);
}

int lograst_forward_project(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                            const float* rotations, const float* opacities, const float* colors,
                            int32_t* radii, void* geom, void* tile_state, uint32_t* num_instances_host,
                            uint32_t* max_tile_len_host, void* stream) {
  LrForwardArgs a = {view, n, means3d, scales, rotations, opacities, colors, radii, geom, tile_state};
  a.stream = stream;
  int rc = lr_forward(a, true, false);
  if (rc) return rc;
  if (num_instances_host || max_tile_len_host) {
    hipStream_t s = (hipStream_t)stream;
    uint32_t hdr[LR_HDR_WORDS] = {0};
    LR_HIP(hipMemcpyAsync(hdr, tile_state, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, s));
    LR_HIP(hipStreamSynchronize(s));
    if (num_instances_host) *num_instances_host = hdr[LR_HDR_NUM];
    if (max_tile_len_host) *max_tile_len_host = hdr[LR_HDR_MAXLEN];
  }
  return LOGRAST_OK;
}

int lograst_forward_render(const lograst_view* view, int32_t n, const void* geom, void* tile_state,
                           uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                           float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                           float* point_weight_pixel, float* point_weight, float* bwd_scratch,
                           int32_t bwd_scratch_floats, uint32_t* status, void* stream) {
  const LrForwardArgs a = {view, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(geom), tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward(a, false, true);
}

int lograst_forward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                    const float* rotations, const float* opacities, const float* colors, int32_t* radii, void* geom,
                    void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                    float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                    float* point_weight_pixel, float* point_weight, float* bwd_scratch, int32_t bwd_scratch_floats,
                    uint32_t* status, void* stream) {
  const LrForwardArgs a = {view, n, means3d, scales, rotations, opacities, colors, radii, geom, tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward(a, true, true);
}

// ---- aux channels: the forward entry points once more, with a second colour triple per Gaussian ----------------------
static LrForwardArgs lr_with_aux(LrForwardArgs a, const float* aux_colors, float* aux_image) {
  a.aux = 1; a.aux_colors = aux_colors; a.aux_image = aux_image;
  return a;
}
int lograst_forward_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                        const float* rotations, const float* opacities, const float* colors, int32_t* radii, void* geom,
                        void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                        float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                        float* point_weight_pixel, float* point_weight, float* bwd_scratch, int32_t bwd_scratch_floats,
                        uint32_t* status, const float* aux_colors, float* aux_image, void* stream) {
  const LrForwardArgs a = {view, n, means3d, scales, rotations, opacities, colors, radii, geom, tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward(lr_with_aux(a, aux_colors, aux_image), true, true);
}
int lograst_forward_render_aux(const lograst_view* view, int32_t n, const void* geom, void* tile_state,
                               uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                               float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                               float* point_weight_pixel, float* point_weight, float* bwd_scratch,
                               int32_t bwd_scratch_floats, uint32_t* status, const float* aux_colors, float* aux_image,
                               void* stream) {
  const LrForwardArgs a = {view, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(geom), tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward(lr_with_aux(a, aux_colors, aux_image), false, true);
}

// The stage-2 outputs of a forward once more, for other colours, from the lists of a forward that ran: no fill, no sort.
int lograst_recomposite(const lograst_view* view, int32_t n, const int32_t* radii, const void* geom, const void* tile_state,
                        const uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len, const float* colors,
                        void* records, int32_t* radii_out, float* image, float* final_t, int32_t* n_contrib,
                        int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight, float* bwd_scratch,
                        int32_t bwd_scratch_floats, uint32_t* status, void* stream) {
  const LrForwardArgs a = {view, n, nullptr, nullptr, nullptr, nullptr, colors, const_cast<int32_t*>(radii), records,
                           const_cast<void*>(tile_state), nullptr, const_cast<uint32_t*>(point_list), capacity, max_tile_len,
                           image, final_t, n_contrib, point_id_pixel, point_weight_pixel, point_weight, bwd_scratch,
                           bwd_scratch_floats, status, stream};
  g_prof_call++;
  LrView v;
  int rc = lr_make_view(view, &v);
  if (rc) return rc;
  if ((rc = lr_check_stage2_args(v, a, false))) return rc;
  if (n > 0 && (!radii || !geom || !colors || !records || !radii_out)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if ((reinterpret_cast<uintptr_t>(geom) | reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(tile_state)) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, "geom / records / tile_state must be 16-byte aligned");
  if (n > 0 && records == geom) return lr_fail(LOGRAST_ERR_ARG, "records must not be the first forward's geom (its backward still reads it)");
  if (v.ty0 != 0 || v.ty1 != v.gy) return lr_fail(LOGRAST_ERR_ARG, "lograst_recomposite renders whole images only (tile_row_begin / tile_row_end)");
  const LrPlan p = lr_plan(v, n);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* st = reinterpret_cast<uint32_t*>(a.tile_state);   // (written by the compositing kernels only with what it holds: open[], LR_HDR_OPEN)
  if (n == 0 && status)   // no recolour kernel runs: this pass's entries of the status block
    LR_HIP(hipMemsetAsync(status + LOGRAST_STATUS_LAST_INSTANCES, 0, 4 * sizeof(uint32_t), s));
  const LrCompositePlan c = lr_composite_plan(v, p, a);
  lr_launch_recolor(n, radii, geom, colors, records, radii_out, c.zero_n, c.zero_block, st, status, s);
  lr_composite(v, p, a, records, c, st, false, s);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

// Side stream + event + pinned words for the read-back of lograst_forward_speculative, one set per host thread and
// device (created on first use, never destroyed: they live as long as the process).
struct LrSpec { int dev; hipStream_t side; hipEvent_t ev; uint32_t* pinned; };
static thread_local std::vector<LrSpec> g_spec;
static int lr_spec_get(LrSpec** out) {
  int dev = 0;
  LR_HIP(hipGetDevice(&dev));
  for (auto& e : g_spec)
    if (e.dev == dev) { *out = &e; return LOGRAST_OK; }
  LrSpec e{dev, nullptr, nullptr, nullptr};
  LR_HIP(hipStreamCreateWithFlags(&e.side, hipStreamNonBlocking));
  LR_HIP(hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));
  LR_HIP(hipHostMalloc(reinterpret_cast<void**>(&e.pinned), sizeof(uint32_t) * LR_HDR_WORDS, hipHostMallocDefault));
  g_spec.push_back(e);
  *out = &g_spec.back();
  return LOGRAST_OK;
}

static int lr_forward_speculative(LrForwardArgs a, uint32_t* num_instances_host, uint32_t* max_tile_len_host) {
  void* const tile_state = a.tile_state;
  LrView v;
  int rc = lr_forward_check(a, true, true, &v);
  if (rc) return rc;
  if (!num_instances_host || !max_tile_len_host) return lr_fail(LOGRAST_ERR_ARG, "NULL host pointer");
  LrSpec* sp = nullptr;
  rc = lr_spec_get(&sp);
  if (rc) return rc;
  // stage 2 is enqueued before the host knows whether `capacity` suffices: the stream never waits for the host ...
  a.speculative = 1;
  a.after_stage1 = sp->ev;   // the scan has written the header: instance count and longest list
  rc = lr_forward_launch(v, a, true, true);
  if (rc) return rc;
  // ... and the header is read on a side stream that waits for stage 1 only (the fill kernel rewrites only the overflow
  // word, which is not read here)
  LR_HIP(hipStreamWaitEvent(sp->side, sp->ev, 0));
  LR_HIP(hipMemcpyAsync(sp->pinned, tile_state, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, sp->side));
  LR_HIP(hipStreamSynchronize(sp->side));
  *num_instances_host = sp->pinned[LR_HDR_NUM];
  *max_tile_len_host = sp->pinned[LR_HDR_MAXLEN];
  return LOGRAST_OK;
}
int lograst_forward_speculative(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                const float* rotations, const float* opacities, const float* colors, int32_t* radii,
                                void* geom, void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity,
                                uint32_t max_tile_len, float* image, float* final_t, int32_t* n_contrib,
                                int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight,
                                float* bwd_scratch, int32_t bwd_scratch_floats, uint32_t* status,
                                uint32_t* num_instances_host, uint32_t* max_tile_len_host, void* stream) {
  const LrForwardArgs a = {view, n, means3d, scales, rotations, opacities, colors, radii, geom, tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward_speculative(a, num_instances_host, max_tile_len_host);
}
int lograst_forward_speculative_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                    const float* rotations, const float* opacities, const float* colors, int32_t* radii,
                                    void* geom, void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity,
                                    uint32_t max_tile_len, float* image, float* final_t, int32_t* n_contrib,
                                    int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight,
                                    float* bwd_scratch, int32_t bwd_scratch_floats, uint32_t* status, const float* aux_colors,
                                    float* aux_image, uint32_t* num_instances_host, uint32_t* max_tile_len_host, void* stream) {
  const LrForwardArgs a = {view, n, means3d, scales, rotations, opacities, colors, radii, geom, tile_state,
                           keys, point_list, capacity, max_tile_len, image, final_t, n_contrib, point_id_pixel,
                           point_weight_pixel, point_weight, bwd_scratch, bwd_scratch_floats, status, stream};
  return lr_forward_speculative(lr_with_aux(a, aux_colors, aux_image), num_instances_host, max_tile_len_host);
}

int lograst_tile_rows(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                      const float* rotations, uint32_t* rows_out, void* stream) {
  g_prof_call++;
  LrView v;
  int rc = lr_make_view(view, &v);
  if (rc) return rc;
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (n == 0) return LOGRAST_OK;
  if (!means3d || !rows_out || (!v.cov3d && (!scales || !rotations))) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (reinterpret_cast<uintptr_t>(rotations) & 15u) return lr_fail(LOGRAST_ERR_ARG, "rotations must be 16-byte aligned");
  v.ty0 = 0; v.ty1 = v.gy;   // always the rows of the whole image: the caller intersects them with its band
  lr_launch_tile_rows(v, n, means3d, scales, rotations, rows_out, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

size_t lograst_sparse_segment_floats(int32_t kmax) {
  const size_t k = kmax > 0 ? (size_t)kmax : 0;
  return 16 + 16 * k + ((k + 15) / 16) * 16;
}
static int lr_pack_rows_checked(const char* who, float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                                uint32_t* overflow, int clear, const uint32_t* hint, int64_t hint_rows, void* stream) {
  if (groups < 0 || rows_per_group < 0 || kmax <= 0 || hint_rows < 0) return lr_fail(LOGRAST_ERR_ARG, std::string(who) + ": negative size or kmax <= 0");
  if (groups == 0 || rows_per_group == 0) return LOGRAST_OK;
  if (!rows || !packed) return lr_fail(LOGRAST_ERR_ARG, std::string(who) + ": NULL pointer");
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(packed)) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, std::string(who) + ": rows / packed must be 16-byte aligned");
  if (rows_per_group > 0x7fffffffLL) return lr_fail(LOGRAST_ERR_ARG, std::string(who) + ": rows_per_group exceeds 31 bits (int32 row indices)");
  lx_launch_pack_rows(rows, groups, rows_per_group, kmax, packed, lograst_sparse_segment_floats(kmax), overflow, clear, hint,
                      hint_rows, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_pack_rows(const float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                      uint32_t* overflow, void* stream) {
  return lr_pack_rows_checked("lograst_pack_rows", const_cast<float*>(rows), groups, rows_per_group, kmax, packed, overflow, 0, nullptr, 0, stream);
}
int lograst_pack_rows_clear(float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                            uint32_t* overflow, void* stream) {
  return lr_pack_rows_checked("lograst_pack_rows_clear", rows, groups, rows_per_group, kmax, packed, overflow, 1, nullptr, 0, stream);
}
int lograst_pack_rows_hinted(float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                             uint32_t* overflow, int32_t clear, const uint32_t* hint, int64_t hint_rows, void* stream) {
  if (!hint) return lr_fail(LOGRAST_ERR_ARG, "lograst_pack_rows_hinted: NULL hint (use lograst_pack_rows / lograst_pack_rows_clear)");
  return lr_pack_rows_checked("lograst_pack_rows_hinted", rows, groups, rows_per_group, kmax, packed, overflow, clear ? 1 : 0, hint,
                              hint_rows, stream);
}
int lograst_add_visible(float* seen, const int32_t* radii, int64_t n, void* stream) {
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "lograst_add_visible: negative n");
  if (n == 0) return LOGRAST_OK;
  if (!seen || !radii) return lr_fail(LOGRAST_ERR_ARG, "lograst_add_visible: NULL pointer");
  lx_launch_add_visible(seen, radii, n, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_add_visible_n(float* seen, const int32_t* const* radii, int32_t k, int64_t n, void* stream) {
  if (n < 0 || k < 0 || k > 16) return lr_fail(LOGRAST_ERR_ARG, "lograst_add_visible_n: negative n, or k outside 0..16");
  if (n == 0 || k == 0) return LOGRAST_OK;
  if (!seen || !radii) return lr_fail(LOGRAST_ERR_ARG, "lograst_add_visible_n: NULL pointer");
  for (int j = 0; j < k; j++)
    if (!radii[j]) return lr_fail(LOGRAST_ERR_ARG, "lograst_add_visible_n: NULL radii pointer");
  lx_launch_add_visible_n(seen, radii, k, n, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_unpack_rows(float* dest, const float* packed, int32_t segments, int32_t kmax, int64_t rows_per_group,
                        int64_t dest_group_rows, int32_t atomic, void* stream) {
  if (segments < 0 || kmax <= 0 || rows_per_group < 0 || dest_group_rows < 0)
    return lr_fail(LOGRAST_ERR_ARG, "lograst_unpack_rows: negative size or kmax <= 0");
  if (segments == 0 || rows_per_group == 0) return LOGRAST_OK;
  if (!dest || !packed) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if ((reinterpret_cast<uintptr_t>(dest) | reinterpret_cast<uintptr_t>(packed)) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, "lograst_unpack_rows: dest / packed must be 16-byte aligned");
  if (atomic != 1 && dest_group_rows < rows_per_group)
    return lr_fail(LOGRAST_ERR_ARG, "lograst_unpack_rows: dest_group_rows must cover rows_per_group (segment s owns rows [s * dest_group_rows, ...))");
  if (atomic < 0 || atomic > 2) return lr_fail(LOGRAST_ERR_ARG, "lograst_unpack_rows: atomic is 0 (store), 1 (add) or 2 (zero the named rows)");
  lx_launch_unpack_rows(dest, packed, segments, kmax, lograst_sparse_segment_floats(kmax), rows_per_group,
                        atomic == 1 ? 0 : dest_group_rows, atomic == 1, atomic == 2, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

int lograst_stream_copy(void* dst, const void* src, size_t bytes, int32_t blocks, void* stream) {
  if (bytes && (!dst || !src)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | bytes) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, "lograst_stream_copy: pointers and size must be multiples of 16 bytes");
  lr_launch_stream_copy(src, dst, bytes, blocks, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

int lograst_knob_count(void) { return LRKNOB_COUNT; }
int lograst_knob_info(int32_t index, const char** name, int32_t* dflt, int32_t* lo, int32_t* hi, const char** what) {
  if (index < 0 || index >= LRKNOB_COUNT) return lr_fail(LOGRAST_ERR_ARG, "knob index out of range");
  if (name) *name = kKnobs[index].name;
  if (dflt) *dflt = kKnobs[index].dflt;
  if (lo) *lo = kKnobs[index].lo;
  if (hi) *hi = kKnobs[index].hi;
  if (what) *what = kKnobs[index].what;
  return LOGRAST_OK;
}
static const LrKnobInfo* lr_find_knob(const char* name) {
  if (!name) return nullptr;
  for (const LrKnobInfo& k : kKnobs)
    if (std::strcmp(k.name, name) == 0) return &k;
  return nullptr;
}
int lograst_set_knob(const char* name, int32_t value) {
  const LrKnobInfo* k = lr_find_knob(name);
  if (!k) return lr_fail(LOGRAST_ERR_ARG, std::string("unknown knob: ") + (name ? name : "(null)"));
  if (value < k->lo || value > k->hi) return lr_fail(LOGRAST_ERR_ARG, std::string(name) + ": value out of range");
  std::lock_guard<std::mutex> lk(g_knob_mu);
  g_knob_set[k->id] = true;
  g_knob_over[k->id] = value;
  lr_resolve_knobs_locked();
  return LOGRAST_OK;
}
int lograst_get_knob(const char* name, int32_t* value) {
  const LrKnobInfo* k = lr_find_knob(name);
  if (!k || !value) return lr_fail(LOGRAST_ERR_ARG, "unknown knob or NULL pointer");
  *value = lr_knob(k->id);
  return LOGRAST_OK;
}
int lograst_reset_knobs(void) {
  std::lock_guard<std::mutex> lk(g_knob_mu);
  for (bool& set : g_knob_set) set = false;
  lr_resolve_knobs_locked();
  return LOGRAST_OK;
}

int lograst_set_tile_cull(int enabled) {
  const int old = lr_tile_cull();
  g_tile_cull.store(enabled ? 1 : 0, std::memory_order_relaxed);
  return old;
}

int lograst_read_state(const void* tile_state, uint32_t* num_instances_host, uint32_t* overflow_host,
                       uint32_t* max_tile_len_host, uint32_t* rect_instances_host, void* stream) {
  if (!tile_state) return lr_fail(LOGRAST_ERR_ARG, "tile_state is NULL");
  uint32_t hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t s = (hipStream_t)stream;
  LR_HIP(hipMemcpyAsync(hdr, tile_state, sizeof(hdr), hipMemcpyDeviceToHost, s));
  LR_HIP(hipStreamSynchronize(s));
  if (num_instances_host) *num_instances_host = hdr[LR_HDR_NUM];
  if (overflow_host) *overflow_host = hdr[LR_HDR_OVERFLOW];
  if (max_tile_len_host) *max_tile_len_host = hdr[LR_HDR_MAXLEN];
  if (rect_instances_host) *rect_instances_host = hdr[LR_HDR_RECT];
  return LOGRAST_OK;
}

// What lograst_backward_aux has on top of lograst_backward.
struct LrAuxGrads { const float *aux_colors, *dl_daux_image; int32_t bwd_row_floats; float* dl_daux_colors; };
// What the *_camera entry points have on top: dL/dviewmatrix and dL/dprojmatrix [4, 4] and the chain rule's partials scratch.
struct LrCameraOut { float *dl_dview, *dl_dproj; void* scratch; size_t scratch_bytes; };
// What the four backward entry points share: the parameters of lograst_backward (include/lograst.h), in its order, so that an
// entry point fills it with one braced list; then which entry point it is and what it has on top (NULL / 0: off).
enum LrBackwardExtra { LR_BWD_PLAIN = 0, LR_BWD_AUX, LR_BWD_CAMERA, LR_BWD_ABS };
struct LrBackwardArgs {
  const lograst_view* view; int32_t n;
  const float *means3d, *scales, *rotations; const int32_t* radii; const void *geom, *tile_state; const uint32_t* point_list;
  const float* final_t; const int32_t* n_contrib; const float* dl_dimage;
  float *dl_dmeans2d, *bwd_rows, *dl_dopacities, *dl_dcolors, *dl_dmeans3d, *dl_dscales, *dl_drotations;
  const float* point_weight; int32_t flags; void* stream;
  LrBackwardExtra extra;
  LrAuxGrads aux;           // lograst_backward_aux
  LrCameraOut cam;          // lograst_backward_camera
  float* dl_dmeans2d_abs;   // lograst_backward_abs: [n, 3]
};
// lograst_project_backward's parameters in its order, and the camera form's on top.
struct LrProjectBackwardArgs {
  const lograst_view* view; int32_t n;
  const float *means3d, *scales, *rotations; const int32_t* radii; const float *dl_dmeans2d, *dl_dconic;
  float *dl_dmeans3d, *dl_dscales, *dl_drotations; void* stream;
  bool camera; LrCameraOut cam;
};

// What the extras refuse alike -- running sums, the cov3d_precomp form, a band view -- each in the caller's words (NULL: that
// one is not this call's to refuse here).
static int lr_refuse_forms(const LrView& v, int32_t flags, const char* sums, const char* cov3d, const char* band) {
  if (sums && (flags & (LOGRAST_BWD_ACCUMULATE | LOGRAST_BWD_ACCUMULATE_ROWS))) return lr_fail(LOGRAST_ERR_ARG, sums);
  if (cov3d && v.cov3d) return lr_fail(LOGRAST_ERR_ARG, cov3d);
  if (band && (v.ty0 != 0 || v.ty1 != v.gy)) return lr_fail(LOGRAST_ERR_ARG, band);
  return LOGRAST_OK;
}
// The camera form's own argument errors, before any launch; *done: n == 0, the two gradients are zeros and nothing else is to do.
static int lr_check_camera(const LrView& v, int32_t n, int32_t flags, const LrCameraOut& cam, hipStream_t s, bool* done) {
  *done = false;
  if (!cam.dl_dview || !cam.dl_dproj) return lr_fail(LOGRAST_ERR_ARG, "dl_dviewmatrix / dl_dprojmatrix are NULL");
  if (int rc = lr_refuse_forms(v, flags, "camera gradients come with fresh gradients only (no LOGRAST_BWD_ACCUMULATE / _ROWS form)",
                               "camera gradients have no cov3d_precomp form",
                               "camera gradients are summed over whole images only (tile_row_begin / tile_row_end)"))
    return rc;
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (n == 0) {
    LR_HIP(hipMemsetAsync(cam.dl_dview, 0, 16 * sizeof(float), s));
    LR_HIP(hipMemsetAsync(cam.dl_dproj, 0, 16 * sizeof(float), s));
    *done = true;
    return LOGRAST_OK;
  }
  if (!cam.scratch || cam.scratch_bytes < lr_camera_scratch_bytes(n))
    return lr_fail(LOGRAST_ERR_ARG, "camera scratch is NULL or smaller than lograst_camera_scratch_bytes(n)");
  if (reinterpret_cast<uintptr_t>(cam.scratch) & 7u) return lr_fail(LOGRAST_ERR_ARG, "camera scratch must be 8-byte aligned");
  return LOGRAST_OK;
}
// The one backward body behind lograst_backward, lograst_backward_aux, lograst_backward_camera and lograst_backward_abs.
static int lr_backward(const LrBackwardArgs& a) {
  const int32_t n = a.n, flags = a.flags;
  float* const dl_dconic = a.bwd_rows;   // (the fourth gradient argument: since version 3 the n x 16 accumulator rows)
  const bool aux = a.extra == LR_BWD_AUX, camera = a.extra == LR_BWD_CAMERA, abs_sums = a.extra == LR_BWD_ABS;
  hipStream_t s = (hipStream_t)a.stream;
  g_prof_call++;
  LrView v;
  int rc = lr_make_view(a.view, &v);
  if (rc) return rc;
  if (camera) {
    bool done;
    if ((rc = lr_check_camera(v, n, flags, a.cam, s, &done)) || done) return rc;
  }
  if (abs_sums) {   // (the abs form's own argument errors: before anything else of the call, n == 0 included)
    if (!a.dl_dmeans2d_abs) return lr_fail(LOGRAST_ERR_ARG, "dl_dmeans2d_abs is NULL");
    if ((rc = lr_refuse_forms(v, flags, "lograst_backward_abs writes fresh gradients (no LOGRAST_BWD_ACCUMULATE / _ROWS form)",
                              "lograst_backward_abs has no cov3d_precomp form",
                              "lograst_backward_abs: whole images only (tile_row_begin / tile_row_end)")))
      return rc;
  }
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (n == 0) return LOGRAST_OK;
  const bool sink_rows = (flags & LOGRAST_BWD_ACCUMULATE_ROWS) != 0;
  if (aux) {   // (before anything else of the call: the aux form's own argument errors; band and cov3d in the forward's words)
    if ((rc = lr_check_aux_view(v))) return rc;
    if (!a.aux.aux_colors || !a.aux.dl_daux_colors) return lr_fail(LOGRAST_ERR_ARG, "aux_colors / dl_daux_colors are NULL");
    if (!a.dl_dimage && !a.aux.dl_daux_image) return lr_fail(LOGRAST_ERR_ARG, "dl_dimage and dl_daux_image are both NULL");
    if (a.aux.bwd_row_floats != LOGRAST_BWD_ROW_FLOATS)
      return lr_fail(LOGRAST_ERR_ARG, "bwd_rows must hold LOGRAST_BWD_ROW_FLOATS (16) floats per Gaussian (dL/daux_colors: slots 9..11)");
    if ((rc = lr_refuse_forms(v, flags, "lograst_backward_aux writes fresh gradients (no LOGRAST_BWD_ACCUMULATE / _ROWS form)",
                              nullptr, nullptr)))
      return rc;
  }
  if (!a.means3d || !a.radii || !a.geom || !a.tile_state || !a.final_t || !a.n_contrib || (!aux && !a.dl_dimage) ||
      !a.dl_dmeans2d || !dl_dconic || !a.dl_dmeans3d || (!sink_rows && (!a.dl_dopacities || !a.dl_dcolors)))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (sink_rows) {   // dl_dmeans3d = the caller's [n][LOGRAST_GRAD_ROW_FLOATS] running sums; the other four are not used
    if (v.cov3d) return lr_fail(LOGRAST_ERR_ARG, "LOGRAST_BWD_ACCUMULATE_ROWS has no cov3d_precomp form");
    if (!a.scales || !a.rotations) return lr_fail(LOGRAST_ERR_ARG, "scales / rotations are NULL");
    if (reinterpret_cast<uintptr_t>(a.dl_dmeans3d) & 63u)
      return lr_fail(LOGRAST_ERR_ARG, "LOGRAST_BWD_ACCUMULATE_ROWS: the gradient rows must be 64-byte aligned");
    if (reinterpret_cast<uintptr_t>(a.rotations) & 15u) return lr_fail(LOGRAST_ERR_ARG, "rotations must be 16-byte aligned");
  } else {
    rc = lr_check_cov_args(v, a.scales, a.rotations, a.dl_dscales, a.dl_drotations);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(a.rotations) | reinterpret_cast<uintptr_t>(a.dl_drotations)) & 15u)
      return lr_fail(LOGRAST_ERR_ARG, "rotations / dl_drotations must be 16-byte aligned");
  }
  if (reinterpret_cast<uintptr_t>(a.bwd_rows) & 63u)
    return lr_fail(LOGRAST_ERR_ARG, "bwd_rows must be 64-byte aligned (one accumulator row per line)");
  if ((flags & LOGRAST_BWD_CONIC_TOUCHED_ONLY) && !a.point_weight)
    return lr_fail(LOGRAST_ERR_ARG, "LOGRAST_BWD_CONIC_TOUCHED_ONLY needs point_weight");
  // A forward with extras on a large input clears the dL/dconic rows of contributing Gaussians only (lr_stage2:
  // touched_only); the chain rule must then skip the others, which it does exactly when it is handed point_weight.
  const bool big_input = lr_big_input(n);
  if ((flags & LOGRAST_BWD_SCRATCH_ZEROED) && v.extras && big_input && !a.point_weight)
    return lr_fail(LOGRAST_ERR_ARG, "LOGRAST_BWD_SCRATCH_ZEROED after a forward with view.extras and n >= "
                                    "LOGRAST_HELPER_MIN_N: dL/dconic is cleared for contributing Gaussians only, pass "
                                    "point_weight (+ LOGRAST_BWD_CONIC_TOUCHED_ONLY)");
  if (!(flags & LOGRAST_BWD_SCRATCH_ZEROED))
    LR_HIP(hipMemsetAsync(dl_dconic, 0, sizeof(float) * LOGRAST_BWD_ROW_FLOATS * (size_t)n, s));
  LrBlendBwdArgs w = {};
  w.geom = a.geom; w.state = reinterpret_cast<const uint32_t*>(a.tile_state); w.tiles = (uint32_t)(v.gx * v.gy);
  w.plist = a.point_list; w.capacity = 0xffffffffu;   // capacity check is a forward concern: a list that rendered is by construction within capacity
  w.final_T = a.final_t; w.n_contrib = a.n_contrib; w.dL_dimage = a.dl_dimage; w.acc_rows = dl_dconic;
  w.big_input = big_input ? 1 : 0; w.masks = v.masks; w.aux_colors = a.aux.aux_colors; w.dL_daux = a.aux.dl_daux_image;
  w.abs_sums = abs_sums;
  lr_launch_blend_bwd(v, w, s);
  // the chain rule reads every live Gaussian's accumulator row and hands out the separate outputs: dL/dmeans2D (written
  // for all rows), dL/dopacities and dL/dcolors (written, or added to the caller's running sums)
  LrProjectBwdArgs c = {};
  c.N = n; c.means = a.means3d; c.scales = a.scales; c.rots = a.rotations; c.radii = a.radii; c.rows = dl_dconic;
  c.o_mean2d = a.dl_dmeans2d; c.o_opac = a.dl_dopacities; c.o_col = a.dl_dcolors; c.pw = a.point_weight;
  c.g_means3d = a.dl_dmeans3d; c.g_scales = a.dl_dscales; c.g_rots = a.dl_drotations;
  c.accumulate = (flags & LOGRAST_BWD_ACCUMULATE) != 0 || sink_rows; c.sink_rows = sink_rows; c.big_input = big_input;
  c.o_aux = a.aux.dl_daux_colors; c.o_abs = a.dl_dmeans2d_abs;   // (NULL but for their entry point, like the camera's three)
  c.cam_partials = static_cast<float*>(a.cam.scratch); c.cam_dv = a.cam.dl_dview; c.cam_dp = a.cam.dl_dproj;
  lr_launch_project_bwd(v, c, s);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_backward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                     const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                     const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                     const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                     float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                     const float* point_weight, int32_t flags, void* stream) {
  return lr_backward({view, n, means3d, scales, rotations, radii, geom, tile_state, point_list, final_t, n_contrib, dl_dimage,
                      dl_dmeans2d, bwd_rows, dl_dopacities, dl_dcolors, dl_dmeans3d, dl_dscales, dl_drotations, point_weight,
                      flags, stream});
}
int lograst_backward_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                         const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                         const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                         const float* aux_colors, const float* dl_dimage, const float* dl_daux_image, float* dl_dmeans2d,
                         float* bwd_rows, int32_t bwd_row_floats, float* dl_dopacities, float* dl_dcolors,
                         float* dl_daux_colors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                         const float* point_weight, int32_t flags, void* stream) {
  return lr_backward({view, n, means3d, scales, rotations, radii, geom, tile_state, point_list, final_t, n_contrib, dl_dimage,
                      dl_dmeans2d, bwd_rows, dl_dopacities, dl_dcolors, dl_dmeans3d, dl_dscales, dl_drotations, point_weight,
                      flags, stream, LR_BWD_AUX, {aux_colors, dl_daux_image, bwd_row_floats, dl_daux_colors}});
}

int lograst_backward_camera(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                            const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                            const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                            const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                            float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                            const float* point_weight, int32_t flags, float* dl_dviewmatrix, float* dl_dprojmatrix,
                            void* camera_scratch, size_t camera_scratch_bytes, void* stream) {
  return lr_backward({view, n, means3d, scales, rotations, radii, geom, tile_state, point_list, final_t, n_contrib, dl_dimage,
                      dl_dmeans2d, bwd_rows, dl_dopacities, dl_dcolors, dl_dmeans3d, dl_dscales, dl_drotations, point_weight,
                      flags, stream, LR_BWD_CAMERA, {}, {dl_dviewmatrix, dl_dprojmatrix, camera_scratch, camera_scratch_bytes}});
}
size_t lograst_camera_scratch_bytes(int32_t n) { return lr_camera_scratch_bytes(n); }

int lograst_backward_abs(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                         const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                         const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                         const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                         float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                         const float* point_weight, int32_t flags, float* dl_dmeans2d_abs, void* stream) {
  return lr_backward({view, n, means3d, scales, rotations, radii, geom, tile_state, point_list, final_t, n_contrib, dl_dimage,
                      dl_dmeans2d, bwd_rows, dl_dopacities, dl_dcolors, dl_dmeans3d, dl_dscales, dl_drotations, point_weight,
                      flags, stream, LR_BWD_ABS, {}, {}, dl_dmeans2d_abs});
}

// The one body behind lograst_project_backward and lograst_project_backward_camera.
static int lr_project_backward(const LrProjectBackwardArgs& a) {
  hipStream_t s = (hipStream_t)a.stream;
  g_prof_call++;
  LrView v;
  int rc = lr_make_view(a.view, &v);
  if (rc) return rc;
  if (a.camera) {
    bool done;
    if ((rc = lr_check_camera(v, a.n, 0, a.cam, s, &done)) || done) return rc;
  }
  if (a.n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (a.n == 0) return LOGRAST_OK;
  if (!a.means3d || !a.radii || !a.dl_dmeans2d || !a.dl_dconic || !a.dl_dmeans3d)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  rc = lr_check_cov_args(v, a.scales, a.rotations, a.dl_dscales, a.dl_drotations);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(a.dl_dconic) | reinterpret_cast<uintptr_t>(a.rotations) |
       reinterpret_cast<uintptr_t>(a.dl_drotations)) & 15u)
    return lr_fail(LOGRAST_ERR_ARG, "rotations / dl_dconic / dl_drotations must be 16-byte aligned");
  LrProjectBwdArgs c = {};
  c.N = a.n; c.means = a.means3d; c.scales = a.scales; c.rots = a.rotations; c.radii = a.radii;
  c.g_mean2d = a.dl_dmeans2d; c.g_conic = a.dl_dconic;
  c.g_means3d = a.dl_dmeans3d; c.g_scales = a.dl_dscales; c.g_rots = a.dl_drotations;
  c.cam_partials = static_cast<float*>(a.cam.scratch); c.cam_dv = a.cam.dl_dview; c.cam_dp = a.cam.dl_dproj;   // (NULL without camera)
  lr_launch_project_bwd(v, c, s);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}
int lograst_project_backward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                             const float* rotations, const int32_t* radii, const float* dl_dmeans2d,
                             const float* dl_dconic, float* dl_dmeans3d, float* dl_dscales,
                             float* dl_drotations, void* stream) {
  return lr_project_backward({view, n, means3d, scales, rotations, radii, dl_dmeans2d, dl_dconic, dl_dmeans3d, dl_dscales,
                              dl_drotations, stream});
}
int lograst_project_backward_camera(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                    const float* rotations, const int32_t* radii, const float* dl_dmeans2d,
                                    const float* dl_dconic, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                                    float* dl_dviewmatrix, float* dl_dprojmatrix, void* camera_scratch,
                                    size_t camera_scratch_bytes, void* stream) {
  return lr_project_backward({view, n, means3d, scales, rotations, radii, dl_dmeans2d, dl_dconic, dl_dmeans3d, dl_dscales,
                              dl_drotations, stream, true, {dl_dviewmatrix, dl_dprojmatrix, camera_scratch, camera_scratch_bytes}});
}

size_t lograst_knn_scratch_bytes(int32_t p) { return lr_knn_scratch_bytes(p); }

int lograst_knn_mean_dist2(int32_t p, const float* points, float* out, void* scratch, size_t scratch_bytes,
                           void* stream) {
  if (p < 0) return lr_fail(LOGRAST_ERR_ARG, "negative point count");
  if (p == 0) return LOGRAST_OK;
  if (!points || !out || !scratch) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (scratch_bytes < lr_knn_scratch_bytes(p)) return lr_fail(LOGRAST_ERR_ARG, "knn scratch too small");
  LR_HIP(lr_launch_knn(p, points, out, scratch, scratch_bytes, (hipStream_t)stream));
  return LOGRAST_OK;
}

size_t lograst_lod_scratch_bytes(int32_t num_roots, int32_t num_nodes, int32_t max_child) {
  return lr_lod_scratch_bytes(num_roots, num_nodes, max_child > 0 ? max_child : 1);
}

int lograst_lod_traverse(int32_t num_points, int32_t num_nodes, int32_t max_child, const int32_t* node_index,
                         const int32_t* tree, const float* xyz, const float* scaling, const float* rotation,
                         const int64_t* root_index, int32_t num_roots, const float* projmatrix,
                         const float* viewmatrix, float focal_x, float focal_y, float tanfovx, float tanfovy,
                         float min_resolution_pixel, int32_t levels, int64_t* out_index, uint32_t out_capacity,
                         void* scratch, size_t scratch_bytes, void* stream) {
  if (num_points < 0 || num_nodes < 0 || num_roots < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (max_child < 1) return lr_fail(LOGRAST_ERR_ARG, "max_child must be >= 1");
  if ((uint64_t)num_nodes * (uint64_t)max_child > 0x7fffffffull) return lr_fail(LOGRAST_ERR_ARG, "tree too large");
  if (!scratch || scratch_bytes < lr_lod_scratch_bytes(num_roots, num_nodes, max_child))
    return lr_fail(LOGRAST_ERR_ARG, "lod scratch too small");
  if (num_roots > 0 && (!root_index || !node_index || !xyz || !scaling || !rotation || !projmatrix || !viewmatrix || !out_index))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (num_nodes > 0 && !tree) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (levels < 0) levels = 0;
  if (levels > lr_lod_max_levels()) levels = lr_lod_max_levels();
  g_prof_call++;
  LR_HIP(lr_launch_lod(num_points, num_nodes, max_child, node_index, tree, xyz, scaling, rotation, root_index, num_roots,
                       projmatrix, viewmatrix, focal_x, focal_y, tanfovx, tanfovy, min_resolution_pixel, levels,
                       out_index, out_capacity, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_lod_read(const void* scratch, uint32_t* count_host, uint32_t* overflow_host, uint32_t* frontier_left_host,
                     void* stream) {
  if (!scratch || !count_host) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  uint32_t w[3] = {0, 0, 0};
  LR_HIP(hipMemcpyAsync(w, reinterpret_cast<const uint32_t*>(scratch) + lr_lod_total_word(), sizeof(w),
                        hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  *count_host = w[0];
  if (overflow_host) *overflow_host = w[1];
  if (frontier_left_host) *frontier_left_host = w[2];
  return LOGRAST_OK;
}

// ---- view preparation (prepare.hip) --------------------------------------------------------------------------
size_t lograst_frustum_scratch_bytes(int32_t n) { return lr_frustum_scratch_bytes(n); }

int lograst_frustum_select(int32_t n, int32_t num_points, const float* xyz, const int32_t* rows, const float* full_proj,
                           double padding, const float* scaling, const float* rotation, const float* opacity,
                           uint8_t* flag_out, int64_t* pos_out, int64_t* row_out, float* xyz_out, float* scaling_out,
                           float* rotation_out, float* opacity_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (n < 0 || num_points < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (!rows && n > num_points) return lr_fail(LOGRAST_ERR_ARG, "more entries than points without a row list");
  if (!scratch || scratch_bytes < lr_frustum_scratch_bytes(n)) return lr_fail(LOGRAST_ERR_ARG, "frustum scratch too small");
  if (n > 0 && (!xyz || !full_proj || !flag_out || !pos_out)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  const bool act = scaling || rotation || opacity || xyz_out || scaling_out || rotation_out || opacity_out;
  if (act && (!scaling || !rotation || !opacity || !xyz_out || !scaling_out || !rotation_out || !opacity_out))
    return lr_fail(LOGRAST_ERR_ARG, "the raw parameters and the four activated outputs go together");
  if (!(padding == padding)) return lr_fail(LOGRAST_ERR_ARG, "padding is NaN");
  g_prof_call++;
  // torch narrows the Python doubles -1 - padding and 1. + padding to the tensor's fp32 before it compares
  LR_HIP(lr_launch_frustum(n, num_points, xyz, rows, full_proj, (float)(-1.0 - padding), (float)(1.0 + padding), scaling,
                           rotation, opacity, flag_out, pos_out, row_out, xyz_out, scaling_out, rotation_out, opacity_out,
                           scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_frustum_read(const void* scratch, uint32_t* count_host, void* stream) {
  if (!scratch || !count_host) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  uint32_t w = 0;
  LR_HIP(hipMemcpyAsync(&w, scratch, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  *count_host = w;
  return LOGRAST_OK;
}

static size_t lr_select_roots_bytes(int32_t num_roots) { return 8 * (((size_t)(num_roots > 0 ? num_roots : 0) + 1) & ~(size_t)1); }

size_t lograst_lod_select_scratch_bytes(int32_t num_roots, int32_t num_nodes, int32_t max_child, uint32_t out_capacity) {
  return lr_lod_scratch_bytes(num_roots, num_nodes, max_child > 0 ? max_child : 1) + lr_select_roots_bytes(num_roots) +
         lr_partition_scratch_bytes(out_capacity);
}

int lograst_lod_select(int32_t num_points, int32_t num_nodes, int32_t max_child, const int32_t* node_index,
                       const int32_t* tree, const int8_t* depth, const float* xyz, const float* scaling,
                       const float* rotation, const int64_t* root_rows, int32_t num_roots, const float* root_weight,
                       const int64_t* root_pos, uint8_t* root_flag, int32_t num_root_flags, const float* projmatrix,
                       const float* viewmatrix, float focal_x, float focal_y, float tanfovx, float tanfovy,
                       float min_resolution_pixel, int32_t levels, int32_t opt_all_levels, int32_t current_depth,
                       int64_t* out_index, uint32_t out_capacity, int64_t* out_leaf, int64_t* out_node, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (num_points < 0 || num_nodes < 0 || num_roots < 0 || num_root_flags < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (max_child < 1) return lr_fail(LOGRAST_ERR_ARG, "max_child must be >= 1");
  if ((uint64_t)num_nodes * (uint64_t)max_child > 0x7fffffffull) return lr_fail(LOGRAST_ERR_ARG, "tree too large");
  if (!scratch || scratch_bytes < lograst_lod_select_scratch_bytes(num_roots, num_nodes, max_child, out_capacity))
    return lr_fail(LOGRAST_ERR_ARG, "lod scratch too small");
  if (num_roots > 0 && (!root_rows || !node_index || !depth || !xyz || !scaling || !rotation || !projmatrix || !viewmatrix ||
                        !out_index || !out_leaf || !out_node))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (num_nodes > 0 && !tree) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (root_weight && num_roots > 0 && (!root_pos || !root_flag)) return lr_fail(LOGRAST_ERR_ARG, "root_weight needs root_pos and root_flag");
  if (levels < 0) levels = 0;
  if (levels > lr_lod_max_levels()) levels = lr_lod_max_levels();
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(scratch);
  const size_t lod_bytes = lr_lod_scratch_bytes(num_roots, num_nodes, max_child);
  int64_t* roots = reinterpret_cast<int64_t*>(base + lod_bytes);
  uint32_t* part_chunk = reinterpret_cast<uint32_t*>(base + lod_bytes + lr_select_roots_bytes(num_roots));
  uint32_t* hdr = reinterpret_cast<uint32_t*>(scratch) + lr_lod_total_word();
  g_prof_call++;
  if (root_weight) LR_HIP(lr_launch_root_filter(num_roots, root_rows, root_weight, root_pos, root_flag, num_root_flags, roots, s));
  LR_HIP(lr_launch_lod(num_points, num_nodes, max_child, node_index, tree, xyz, scaling, rotation,
                       root_weight ? roots : root_rows, num_roots, projmatrix, viewmatrix, focal_x, focal_y, tanfovx, tanfovy,
                       min_resolution_pixel, levels, out_index, out_capacity, scratch, s));
  if (num_roots > 0)
    LR_HIP(lr_launch_partition(out_index, hdr, out_capacity, node_index, depth, num_points, opt_all_levels != 0,
                               current_depth, out_leaf, out_node, part_chunk, hdr + 3, s));
  return LOGRAST_OK;
}

int lograst_lod_select_read(const void* scratch, uint32_t* count_all_host, uint32_t* count_leaf_host,
                            uint32_t* overflow_host, uint32_t* frontier_left_host, void* stream) {
  if (!scratch || !count_all_host || !count_leaf_host) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  uint32_t w[4] = {0, 0, 0, 0};
  LR_HIP(hipMemcpyAsync(w, reinterpret_cast<const uint32_t*>(scratch) + lr_lod_total_word(), sizeof(w),
                        hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  *count_all_host = w[0];
  *count_leaf_host = w[3];
  if (overflow_host) *overflow_host = w[1];
  if (frontier_left_host) *frontier_left_host = w[2];
  return LOGRAST_OK;
}

int lograst_clamp_scale(int32_t m, const int64_t* index, const uint8_t* flag, int32_t num_points, float* scaling,
                        const float* radius3d_min, const float* radius3d_max, void* stream) {
  if (m < 0 || num_points < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (m == 0) return LOGRAST_OK;
  if (!index || !scaling || !radius3d_min || !radius3d_max) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_clamp_scale(m, index, flag, num_points, scaling, radius3d_min, radius3d_max, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_init_radius3d(int32_t p, const float* xyz, const float* scaling, const float* rotation, int32_t num_views,
                          const float* cameras, float* radius3d_min, uint8_t* valid, float* radius3d, void* stream) {
  if (p < 0 || num_views < 0) return lr_fail(LOGRAST_ERR_ARG, "negative point or view count");
  if ((valid || radius3d) && num_views != 1)
    return lr_fail(LOGRAST_ERR_ARG, "valid / radius3d are the results of one view: num_views must be 1");
  if (p == 0 || num_views == 0) return LOGRAST_OK;
  if (!xyz || !scaling || !rotation || !cameras) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_init_radius3d(p, xyz, scaling, rotation, num_views, cameras, radius3d_min, valid, radius3d,
                                 (hipStream_t)stream));
  return LOGRAST_OK;
}

size_t lograst_id_histogram_scratch_bytes(int32_t n) { return lr_hist_scratch_bytes(n); }

int lograst_id_histogram(int32_t n, const int32_t* point_id_pixel, int32_t num_pixels, int32_t* ids_out,
                         int64_t* counts_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (n < 0 || num_pixels < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (!scratch || scratch_bytes < lr_hist_scratch_bytes(n)) return lr_fail(LOGRAST_ERR_ARG, "histogram scratch too small");
  if (n > 0 && num_pixels > 0 && (!point_id_pixel || !ids_out || !counts_out)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_id_histogram(n, point_id_pixel, num_pixels, ids_out, counts_out, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_id_histogram_read(const void* scratch, uint32_t* count_host, void* stream) {
  if (!scratch || !count_host) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  LR_HIP(hipMemcpyAsync(count_host, scratch, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_counter_update(int32_t nv, const int64_t* visible_index, const float* grad_means2d, const int32_t* radii,
                           const float* point_weight, int32_t k, const int32_t* point_id, const int64_t* point_count,
                           int32_t num_points, float* weights_max, float* weights_sum, float* grad_sum,
                           int16_t* radii_max, int16_t* visible_count, int32_t* radii_max_max, int32_t* area_sum,
                           int32_t* create_steps, uint8_t* flag_vis_out, void* stream) {
  if (nv < 0 || k < 0 || num_points < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (nv == 0) return LOGRAST_OK;
  if (!visible_index || !grad_means2d || !radii || !point_weight || (k > 0 && (!point_id || !point_count)))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (!weights_max || !weights_sum || !grad_sum || !radii_max || !visible_count || !radii_max_max || !area_sum || !create_steps)
    return lr_fail(LOGRAST_ERR_ARG, "NULL counter buffer");
  CounterArgs a;
  a.visible_index = visible_index; a.grad = grad_means2d; a.radii = radii; a.weight = point_weight;
  a.point_id = point_id; a.point_count = point_count;
  a.weights_max = weights_max; a.weights_sum = weights_sum; a.grad_sum = grad_sum;
  a.radii_max = radii_max; a.visible_count = visible_count;
  a.radii_max_max = radii_max_max; a.area_sum = area_sum; a.create_steps = create_steps;
  a.flag_vis = flag_vis_out;
  a.nv = nv; a.k = k; a.num_points = num_points;
  g_prof_call++;
  LR_HIP(lr_launch_counter(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- fused L1 + SSIM loss (loss.hip) ----------------------------------------------------------------------
// Three forms, one host body per direction: the plain loss; _gain, with the L1 term on gain[b, c] * render (LoG's view
// correction): no render_l1 tensor, one image gradient and the gradient of the gain; _masked, with an ignore mask blended into
// the SSIM input and / or the ground truth composited over a background (the MASKED instantiations).
size_t lograst_loss_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width) {
  return lr_loss_scratch_bytes(batch, channels, height, width);
}

size_t lograst_loss_gain_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width) {
  return lr_loss_gain_scratch_bytes(batch, channels, height, width);
}

size_t lograst_loss_masked_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width) {
  return lr_loss_gain_scratch_bytes(batch, channels, height, width);      // >= lr_loss_scratch_bytes: serves either call
}

// the window: exp(-(x-5)^2 / (2 * 1.5^2)) in double, normalised, rounded to fp32 once (the loss's and the metric's)
static void lr_ssim_window(float* w) {
  double g[LS_WIN_TAPS], sum = 0.0;
  for (int k = 0; k < LS_WIN_TAPS; k++) { g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
  for (int k = 0; k < LS_WIN_TAPS; k++) w[k] = (float)(g[k] / sum);
}

// Inside one image plane the kernels address with 32-bit offsets y * stride_y + x * stride_x (the loss's images and masks, the
// evaluation's images): true when no pixel of the plane lies beyond 2^31 - 1 elements, a negative stride taken by magnitude.
static bool lr_plane_in_32bit(int64_t stride_y, int64_t stride_x, int32_t height, int32_t width) {
  const int64_t sy = stride_y < 0 ? -stride_y : stride_y, sx = stride_x < 0 ? -stride_x : stride_x;
  return sy <= 0x7fffffffLL && sx <= 0x7fffffffLL && (int64_t)(height - 1) * sy + (int64_t)(width - 1) * sx <= 0x7fffffffLL;
}

// What one call of an entry point hands to the shared bodies.  The leading members are what (nearly) every entry point has,
// in the order of its parameters: `LossCall c = {batch, ..., stream}` leaves what follows zero -- a pointer the entry point
// does not have is NULL.
struct LossCall {
  int32_t batch, channels, height, width;
  const float* render; const int64_t* rs;
  const float* render_l1; const int64_t* ls;
  const float* gt; const int64_t* gs;
  const float* gain;
  void* scratch; size_t scratch_bytes;
  void* stream;
  bool gain_required;                                      // _gain: a NULL l1_gain is an error, not the plain loss
  const float* mask; const int64_t* ms;
  const float* fg; const int64_t* fs; const float* bg; float* gt_out;
  size_t scratch_min; const char* scratch_fn;              // the size the entry point accepts, the sizing function its message names
  const char* precondition;                                // the entry point's own precondition that does not hold, or NULL
};

static int lr_loss_scratch(const LossCall& c) {
  if (c.scratch && c.scratch_bytes >= c.scratch_min && !(reinterpret_cast<uintptr_t>(c.scratch) & 7u)) return 0;
  return lr_fail(LOGRAST_ERR_ARG, std::string("loss scratch too small (") + c.scratch_fn + ") or not 8-byte aligned");
}

// Geometry and image checks of both directions; fills the geometry, the images and the window of LossArgs and leaves the
// rest zero.  -> 1 for the empty batch, < 0 after lr_fail.
static int lr_loss_args(LossArgs& a, const LossCall& c) {
  a = LossArgs{};
  if (c.precondition) return lr_fail(LOGRAST_ERR_ARG, c.precondition);
  if (c.batch < 0 || c.channels < 0) return lr_fail(LOGRAST_ERR_ARG, "negative batch or channel count");
  if (c.height < LS_WIN_TAPS || c.width < LS_WIN_TAPS)
    return lr_fail(LOGRAST_ERR_ARG, "image smaller than the 11-pixel window of the SSIM (height and width must be >= 11)");
  if ((int64_t)c.batch * c.channels * (int64_t)c.height * c.width > 0x7fffffffLL)
    return lr_fail(LOGRAST_ERR_ARG, "more than 2^31 - 1 image elements");
  if ((int64_t)c.batch * c.channels == 0) return 1;
  if (!c.render || !c.gt || !c.rs || !c.gs || (c.render_l1 && !c.ls)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  for (const int64_t* st : {c.rs, c.gs, c.render_l1 ? c.ls : c.rs})
    if (!lr_plane_in_32bit(st[2], st[3], c.height, c.width))
      return lr_fail(LOGRAST_ERR_ARG, "y / x strides reach beyond 2^31 - 1 elements inside one image plane");
  bool same = c.render_l1 == c.render;
  for (int i = 0; i < 4; i++) {
    a.rs[i] = c.rs[i]; a.gs[i] = c.gs[i];
    a.ls[i] = c.render_l1 ? c.ls[i] : 0;
    same = same && (!c.render_l1 || c.ls[i] == c.rs[i]);
  }
  a.render = c.render; a.gt = c.gt;
  a.render_l1 = (c.render_l1 && !same) ? c.render_l1 : nullptr;
  a.B = c.batch; a.C = c.channels; a.H = c.height; a.W = c.width;
  lr_ssim_window(a.w);
  return 0;
}

// mask [B, H, W] through three element strides: the same 32-bit in-plane offsets as the images
static int lr_loss_mask_strides(int64_t* dst, const float* p, const int64_t* st, int32_t height, int32_t width, const char* what) {
  if (!p) return 0;
  if (!st) return lr_fail(LOGRAST_ERR_ARG, what);
  if (!lr_plane_in_32bit(st[1], st[2], height, width))
    return lr_fail(LOGRAST_ERR_ARG, "y / x strides reach beyond 2^31 - 1 elements inside one image plane");
  for (int i = 0; i < 3; i++) dst[i] = st[i];
  return 0;
}

static int lr_loss_forward(const LossCall& c, float ssim_weight, float l1_weight, float* out3, float* maps) {
  LossArgs a;
  const int rc = lr_loss_args(a, c);
  if (rc < 0) return rc;
  if (!out3) return lr_fail(LOGRAST_ERR_ARG, "out3 is NULL");
  if (rc == 1) {
    LR_HIP(hipMemsetAsync(out3, 0, 3 * sizeof(float), (hipStream_t)c.stream));
    return LOGRAST_OK;
  }
  if (c.gain_required && !c.gain) return lr_fail(LOGRAST_ERR_ARG, "l1_gain is NULL");
  if (lr_loss_mask_strides(a.ms, c.mask, c.ms, c.height, c.width, "mask without strides") < 0) return LOGRAST_ERR_ARG;
  if (lr_loss_mask_strides(a.fs, c.fg, c.fs, c.height, c.width, "foreground without strides") < 0) return LOGRAST_ERR_ARG;
  if (lr_loss_scratch(c) < 0) return LOGRAST_ERR_ARG;
  a.ntx = (c.width - 10 + 31) / 32; a.nty = (c.height - 10 + 31) / 32;
  const double count = (double)c.batch * c.channels * (double)(c.height - 10) * (double)(c.width - 10);
  a.scale = (float)(-(double)ssim_weight / count);
  a.maps = maps;
  a.partial = reinterpret_cast<float*>(c.scratch);
  a.gain = c.gain;
  a.mask = c.mask; a.fg = c.fg; a.bg = c.fg ? c.bg : nullptr; a.gt_out = c.fg ? c.gt_out : nullptr;
  g_prof_call++;
  LR_HIP(lr_launch_loss_fwd(a, ssim_weight, l1_weight, out3, (hipStream_t)c.stream));
  return LOGRAST_OK;
}

// the scratch holds the partial sums of the gain's gradient: looked at only with a gain
static int lr_loss_backward(const LossCall& c, float l1_weight, const float* grad_loss, const float* maps, float* grad_render,
                            float* grad_render_l1, float* grad_gain) {
  LossArgs a;
  const int rc = lr_loss_args(a, c);
  if (rc < 0) return rc;
  if (rc == 1) return LOGRAST_OK;
  if (!grad_loss || !maps || !grad_render || (c.gain_required && !c.gain) || (c.gain && !grad_gain))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (a.render_l1 && !grad_render_l1) return lr_fail(LOGRAST_ERR_ARG, "render_l1 is a tensor of its own but grad_render_l1 is NULL");
  if (lr_loss_mask_strides(a.ms, c.mask, c.ms, c.height, c.width, "mask without strides") < 0) return LOGRAST_ERR_ARG;
  if (c.gain && lr_loss_scratch(c) < 0) return LOGRAST_ERR_ARG;
  a.ntx = (c.width + 31) / 32; a.nty = (c.height + 31) / 32;
  a.l1_scale = (float)((double)l1_weight / ((double)c.batch * c.channels * (double)c.height * (double)c.width));
  a.maps = const_cast<float*>(maps);
  a.gain = c.gain;
  a.gain_partial = reinterpret_cast<double*>(c.scratch);
  a.mask = c.mask;
  g_prof_call++;
  LR_HIP(lr_launch_loss_bwd(a, grad_loss, grad_render, a.render_l1 ? grad_render_l1 : nullptr, grad_gain, (hipStream_t)c.stream));
  return LOGRAST_OK;
}

int lograst_loss_forward(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                         const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                         const float* gt, const int64_t* gt_strides, float ssim_weight, float l1_weight, float* out3,
                         float* maps, void* scratch, size_t scratch_bytes, void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, render_l1, render_l1_strides, gt, gt_strides, nullptr,
                scratch, scratch_bytes, stream};
  c.scratch_min = lr_loss_scratch_bytes(batch, channels, height, width); c.scratch_fn = "lograst_loss_scratch_bytes";
  return lr_loss_forward(c, ssim_weight, l1_weight, out3, maps);
}

int lograst_loss_backward(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                          const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                          const float* gt, const int64_t* gt_strides, float l1_weight, const float* grad_loss,
                          const float* maps, float* grad_render, float* grad_render_l1, void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, render_l1, render_l1_strides, gt, gt_strides, nullptr,
                nullptr, 0, stream};
  return lr_loss_backward(c, l1_weight, grad_loss, maps, grad_render, grad_render_l1, nullptr);
}

int lograst_loss_forward_gain(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                              const int64_t* render_strides, const float* gt, const int64_t* gt_strides, const float* l1_gain,
                              float ssim_weight, float l1_weight, float* out3, float* maps, void* scratch, size_t scratch_bytes,
                              void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, nullptr, nullptr, gt, gt_strides, l1_gain, scratch, scratch_bytes,
                stream};
  c.gain_required = true;
  // the forward needs the forward's size; the message names the function whose size serves this call and its backward
  c.scratch_min = lr_loss_scratch_bytes(batch, channels, height, width); c.scratch_fn = "lograst_loss_gain_scratch_bytes";
  return lr_loss_forward(c, ssim_weight, l1_weight, out3, maps);
}

int lograst_loss_backward_gain(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                               const int64_t* render_strides, const float* gt, const int64_t* gt_strides, const float* l1_gain,
                               float l1_weight, const float* grad_loss, const float* maps, float* grad_render, float* grad_gain,
                               void* scratch, size_t scratch_bytes, void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, nullptr, nullptr, gt, gt_strides, l1_gain, scratch, scratch_bytes,
                stream};
  c.gain_required = true;
  c.scratch_min = lr_loss_gain_scratch_bytes(batch, channels, height, width); c.scratch_fn = "lograst_loss_gain_scratch_bytes";
  return lr_loss_backward(c, l1_weight, grad_loss, maps, grad_render, nullptr, grad_gain);
}

int lograst_loss_forward_masked(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                                const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                                const float* gt, const int64_t* gt_strides, const float* l1_gain, const float* mask,
                                const int64_t* mask_strides, const float* foreground, const int64_t* foreground_strides,
                                const float* background, float* gt_out, float ssim_weight, float l1_weight, float* out3,
                                float* maps, void* scratch, size_t scratch_bytes, void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, render_l1, render_l1_strides, gt, gt_strides, l1_gain,
                scratch, scratch_bytes, stream};
  c.mask = mask; c.ms = mask_strides; c.fg = foreground; c.fs = foreground_strides; c.bg = background; c.gt_out = gt_out;
  c.scratch_min = lograst_loss_masked_scratch_bytes(batch, channels, height, width); c.scratch_fn = "lograst_loss_masked_scratch_bytes";
  c.precondition = render_l1 && l1_gain ? "render_l1 and l1_gain are mutually exclusive: the L1 term reads one of them"
                   : !mask && !foreground ? "mask and foreground are both NULL: use lograst_loss_forward / _gain"
                   : foreground && (!background || !gt_out) ? "foreground needs background and gt_out" : nullptr;
  return lr_loss_forward(c, ssim_weight, l1_weight, out3, maps);
}

int lograst_loss_backward_masked(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                                 const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                                 const float* gt, const int64_t* gt_strides, const float* l1_gain, const float* mask,
                                 const int64_t* mask_strides, float l1_weight, const float* grad_loss, const float* maps,
                                 float* grad_render, float* grad_render_l1, float* grad_gain, void* scratch, size_t scratch_bytes,
                                 void* stream) {
  LossCall c = {batch, channels, height, width, render, render_strides, render_l1, render_l1_strides, gt, gt_strides, l1_gain,
                scratch, scratch_bytes, stream};
  c.mask = mask; c.ms = mask_strides;
  c.scratch_min = lograst_loss_masked_scratch_bytes(batch, channels, height, width); c.scratch_fn = "lograst_loss_masked_scratch_bytes";
  c.precondition = render_l1 && l1_gain ? "render_l1 and l1_gain are mutually exclusive: the L1 term reads one of them"
                   : !mask ? "mask is NULL: use lograst_loss_backward / _gain on the composited gt" : nullptr;
  return lr_loss_backward(c, l1_weight, grad_loss, maps, grad_render, grad_render_l1, grad_gain);
}

size_t lograst_mask_bounds_bytes(int32_t batch) { return (size_t)(batch > 0 ? batch : 1) * MB_RECORD_INTS * sizeof(int32_t); }

int lograst_mask_bounds(int32_t batch, int32_t height, int32_t width, const float* mask, const int64_t* mask_strides,
                        float threshold, void* record, size_t record_bytes, void* stream) {
  if (batch < 0 || height < 0 || width < 0) return lr_fail(LOGRAST_ERR_ARG, "negative batch, height or width");
  if ((int64_t)batch * height > 0x7fffffffLL) return lr_fail(LOGRAST_ERR_ARG, "more than 2^31 - 1 image rows");
  if (batch == 0) return LOGRAST_OK;
  if (!record || record_bytes < lograst_mask_bounds_bytes(batch) || (reinterpret_cast<uintptr_t>(record) & 3u))
    return lr_fail(LOGRAST_ERR_ARG, "mask bounds record too small (lograst_mask_bounds_bytes) or not 4-byte aligned");
  if ((int64_t)height * width > 0 && (!mask || !mask_strides)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  static const int64_t none[3] = {0, 0, 0};
  LR_HIP(lr_launch_mask_bounds(batch, height, width, mask, mask_strides ? mask_strides : none, threshold,
                               reinterpret_cast<int32_t*>(record), (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_mask_bounds_read(const void* record, int32_t batch, int32_t* host_out, void* stream) {
  if (batch < 0) return lr_fail(LOGRAST_ERR_ARG, "negative batch");
  if (batch == 0) return LOGRAST_OK;
  if (!record || !host_out) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  LR_HIP(hipMemcpyAsync(host_out, record, (size_t)batch * MB_RECORD_INTS * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- fused depth patch loss (depth_loss.hip) --------------------------------------------------------------
size_t lograst_depth_loss_record_bytes(int32_t n) { return lr_depth_loss_record_bytes(n); }

// Checks shared by the two entry points; everything here runs before any device work.
static int lr_depth_loss_args(DepthLossArgs& a, int32_t height, int32_t width, const float* pred, const int64_t* ps,
                              const float* gt, const int64_t* gs, const float* acc, const int64_t* as, int32_t n) {
  if (height < 0 || width < 0) return lr_fail(LOGRAST_ERR_ARG, "negative image size");
  if (height < DL_PATCH || width < DL_PATCH)
    return lr_fail(LOGRAST_ERR_ARG, "image smaller than the 64-pixel patch of the depth loss (height and width must be >= 64)");
  if (n < 1 || n > DL_MAX_PATCHES) return lr_fail(LOGRAST_ERR_ARG, "patch count must be 1..256");
  if (!pred || !gt || !acc || !ps || !gs || !as) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  a.pred = pred; a.gt = gt; a.acc = acc;
  for (int i = 0; i < 2; i++) { a.ps[i] = ps[i]; a.gs[i] = gs[i]; a.as[i] = as[i]; }
  a.H = height; a.W = width;
  return 0;
}

int lograst_depth_loss_forward(int32_t height, int32_t width, const float* pred, const int64_t* pred_strides,
                               const float* gt, const int64_t* gt_strides, const float* acc, const int64_t* acc_strides,
                               int32_t n, const int64_t* rows, const int64_t* cols, double alpha, double eps,
                               double threshold, void* out, void* records, size_t record_bytes, void* stream) {
  DepthLossArgs a;
  const int rc = lr_depth_loss_args(a, height, width, pred, pred_strides, gt, gt_strides, acc, acc_strides, n);
  if (rc < 0) return rc;
  if (!rows || !cols || !out) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (reinterpret_cast<uintptr_t>(out) & 7u) return lr_fail(LOGRAST_ERR_ARG, "out must be 8-byte aligned (float loss at byte 0, double M at byte 8)");
  if (!records || record_bytes < lr_depth_loss_record_bytes(n) || (reinterpret_cast<uintptr_t>(records) & 7u))
    return lr_fail(LOGRAST_ERR_ARG, "depth loss records too small (lograst_depth_loss_record_bytes) or not 8-byte aligned");
  g_prof_call++;
  LR_HIP(lr_launch_depth_loss_fwd(a, n, rows, cols, alpha, eps, threshold, out, reinterpret_cast<double*>(records), (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_depth_loss_backward(int32_t height, int32_t width, const float* pred, const int64_t* pred_strides,
                                const float* gt, const int64_t* gt_strides, const float* acc, const int64_t* acc_strides,
                                int32_t n, const void* records, const float* grad_loss, float* grad_pred, void* stream) {
  DepthLossArgs a;
  const int rc = lr_depth_loss_args(a, height, width, pred, pred_strides, gt, gt_strides, acc, acc_strides, n);
  if (rc < 0) return rc;
  if (!records || !grad_loss || !grad_pred) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (reinterpret_cast<uintptr_t>(records) & 7u) return lr_fail(LOGRAST_ERR_ARG, "depth loss records must be 8-byte aligned");
  g_prof_call++;
  LR_HIP(lr_launch_depth_loss_bwd(a, n, reinterpret_cast<const double*>(records), grad_loss, grad_pred, (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- evaluation: validation metrics and 8-bit export (evaluate.hip) ----------------------------------------
size_t lograst_eval_scratch_bytes(int32_t channels, int32_t height, int32_t width) {
  return lr_eval_scratch_bytes(channels, height, width);
}

// Checks shared by the entry points; everything here runs before any device work.
static int lr_eval_geometry(int32_t channels, int32_t height, int32_t width) {
  if (channels < 1 || channels > 4) return lr_fail(LOGRAST_ERR_ARG, "channels must be 1..4");
  if (height < 1 || width < 1) return lr_fail(LOGRAST_ERR_ARG, "height and width must be at least 1");
  if ((int64_t)channels * (int64_t)height * width > 0x7fffffffLL) return lr_fail(LOGRAST_ERR_ARG, "more than 2^31 - 1 image elements");
  return 0;
}

static int lr_eval_strides(int64_t* dst, const int64_t* st, int32_t height, int32_t width) {
  if (st[1] < 0 || st[2] < 0 || !lr_plane_in_32bit(st[1], st[2], height, width))
    return lr_fail(LOGRAST_ERR_ARG, "y / x strides are negative or reach beyond 2^31 - 1 elements inside one image plane");
  for (int i = 0; i < 3; i++) dst[i] = st[i];
  return 0;
}

int lograst_image_to_bgr8(int32_t channels, int32_t height, int32_t width, const float* image, const int64_t* strides3,
                          uint8_t* out, void* stream) {
  if (lr_eval_geometry(channels, height, width)) return LOGRAST_ERR_ARG;
  if (!image || !strides3 || !out) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (reinterpret_cast<uintptr_t>(out) & 3u) return lr_fail(LOGRAST_ERR_ARG, "out must be 4-byte aligned");
  EvalArgs a = {};
  if (lr_eval_strides(a.ps, strides3, height, width)) return LOGRAST_ERR_ARG;
  a.pred = image; a.C = channels; a.H = height; a.W = width; a.bgr8 = out;
  g_prof_call++;
  LR_HIP(lr_launch_eval_bgr8(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_eval_metrics(int32_t channels, int32_t height, int32_t width, const float* pred, const int64_t* pred_strides3,
                         const float* gt, const int64_t* gt_strides3, int32_t flags, double max_val, float* corrected,
                         uint8_t* bgr8, void* record, void* scratch, size_t scratch_bytes, void* stream) {
  if (lr_eval_geometry(channels, height, width)) return LOGRAST_ERR_ARG;
  if (!pred || !pred_strides3 || !gt || !gt_strides3 || !record) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (flags & ~(LOGRAST_EVAL_FIT_GAIN | LOGRAST_EVAL_SSIM)) return lr_fail(LOGRAST_ERR_ARG, "unknown flag");
  if (reinterpret_cast<uintptr_t>(record) & 7u) return lr_fail(LOGRAST_ERR_ARG, "record must be 8-byte aligned");
  if (!scratch || scratch_bytes < lr_eval_scratch_bytes(channels, height, width) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return lr_fail(LOGRAST_ERR_ARG, "eval scratch too small (lograst_eval_scratch_bytes) or not 8-byte aligned");
  EvalArgs a = {};
  if (lr_eval_strides(a.ps, pred_strides3, height, width) || lr_eval_strides(a.gs, gt_strides3, height, width)) return LOGRAST_ERR_ARG;
  a.pred = pred; a.gt = gt; a.C = channels; a.H = height; a.W = width;
  lr_ssim_window(a.w);
  a.c1 = (float)((0.01 * max_val) * (0.01 * max_val));
  a.c2 = (float)((0.03 * max_val) * (0.03 * max_val));
  a.corrected = corrected; a.bgr8 = bgr8; a.record = reinterpret_cast<double*>(record);
  g_prof_call++;
  LR_HIP(lr_launch_eval_metrics(a, (flags & LOGRAST_EVAL_FIT_GAIN) != 0, (flags & LOGRAST_EVAL_SSIM) != 0, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_eval_read(const void* record, double* out16, void* stream) {
  if (!record || !out16) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  LR_HIP(hipMemcpyAsync(out16, record, 16 * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- the Adam steps over model rows: lograst_sparse_adam, lograst_activate_backward_adam, lograst_accumulated_adam ------
// One key of a step.  Which of `param` (the gathered rows the step starts from) and `grad` the caller's kernel reads differs:
// the fused step has the gradient in registers, the accumulated one reads the model row itself; what is not read is not
// required and not passed on.
static int lr_adam_key(AdamKey& d, const lograst_adam_key& k, bool reads_param, bool reads_grad) {
  if (!k.model_param || (reads_param && !k.param) || (reads_grad && !k.grad) || !k.exp_avg || !k.exp_avg_sq)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer in key");
  d.model = (float*)k.model_param;
  d.param = reads_param ? (const float*)k.param : nullptr;
  d.grad = reads_grad ? (const float*)k.grad : nullptr;
  d.exp_avg = (float*)k.exp_avg; d.exp_avg_sq = (float*)k.exp_avg_sq; d.max_exp_avg_sq = (float*)k.max_exp_avg_sq;
  d.width = k.width; d.neg_step_size = -k.step_size;
  return LOGRAST_OK;
}
// the reference's Python scalars are doubles that torch narrows to fp32 when they meet an fp32 tensor
static void lr_adam_scalars(AdamArgs& a, double beta1, double beta2, double bias_correction2_sqrt, double eps) {
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)bias_correction2_sqrt; a.eps = (float)eps;
}
// widths of the keys of a LoG row in the order of every key list: xyz, scaling, opacity, rotation, colors; shs: 3 * sh_coeffs
static const int kStepKeyWidths[6] = {3, 3, 1, 4, 3, 0};
static int lr_step_key_width(int i, int32_t sh_coeffs) { return i == 5 ? 3 * sh_coeffs : kStepKeyWidths[i]; }

int lograst_sparse_adam(int32_t m, int32_t num_points, const int64_t* index, const uint8_t* flag_vis,
                        int32_t num_keys, const lograst_adam_key* keys, double beta1, double beta2,
                        double bias_correction2_sqrt, double eps, void* stream) {
  if (m < 0 || num_points < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (num_keys < 0 || num_keys > ADAM_MAX_KEYS) return lr_fail(LOGRAST_ERR_ARG, "at most 8 keys per call");
  if (m == 0 || num_keys == 0) return LOGRAST_OK;
  if (!index || !flag_vis || !keys) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < num_keys; i++) {
    int rc = lr_adam_key(a.key[i], keys[i], true, true);
    if (rc) return rc;
    if (keys[i].width < 1) return lr_fail(LOGRAST_ERR_ARG, "key width must be >= 1");
  }
  a.index = index; a.flag_vis = flag_vis; a.m = m; a.num_points = num_points;
  lr_adam_scalars(a, beta1, beta2, bias_correction2_sqrt, eps);
  g_prof_call++;
  LR_HIP(lr_launch_sparse_adam(a, num_keys, (hipStream_t)stream));
  return LOGRAST_OK;
}

// Corrector.step (corrector.py:35-62) for one row of the [views, width] buffers, the step count and the schedule on the device
int lograst_corrector_step(int32_t views, int32_t width, int32_t index, int32_t start_step, double lr_init, double lr_final,
                           int32_t* steps, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                           void* stream) {
  if (views < 1 || width < 1 || width > 64) return lr_fail(LOGRAST_ERR_ARG, "views must be >= 1 and width in 1 .. 64");
  if (index < 0 || index >= views) return lr_fail(LOGRAST_ERR_ARG, "index outside [0, views)");
  if (!(lr_init > 0.0) || !(lr_final > 0.0) || !std::isfinite(lr_init) || !std::isfinite(lr_final))
    return lr_fail(LOGRAST_ERR_ARG, "lr_init and lr_final must be positive and finite");
  if (!steps || !param || !grad || !exp_avg || !exp_avg_sq || !max_exp_avg_sq) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  CorrectorArgs a;
  a.steps = steps; a.param = param; a.grad = grad; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.max_exp_avg_sq = max_exp_avg_sq;
  a.log_lr_init = std::log(lr_init); a.log_lr_final = std::log(lr_final);
  a.index = index; a.width = width; a.start_step = start_step;
  // betas 0.9 / 0.999 and eps 1e-15 of the reference's call, narrowed as lograst_sparse_adam narrows them
  a.beta1 = (float)0.9; a.beta2 = (float)0.999; a.omb1 = (float)(1.0 - 0.9); a.omb2 = (float)(1.0 - 0.999); a.eps = (float)1e-15;
  g_prof_call++;
  LR_HIP(lr_launch_corrector_step(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- per-view pose table (pose.hip) --------------------------------------------------------------------------
static int lr_pose_args(int32_t views, int32_t index, const float* table, const float* viewmatrix, const float* projmatrix) {
  if (views < 1) return lr_fail(LOGRAST_ERR_ARG, "views must be >= 1");
  if (index < 0 || index >= views) return lr_fail(LOGRAST_ERR_ARG, "index outside [0, views)");
  if (!table || !viewmatrix || !projmatrix) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  return LOGRAST_OK;
}
int lograst_pose_apply(int32_t views, int32_t index, const float* table, const float* viewmatrix, const float* projmatrix,
                       float* viewmatrix_out, float* projmatrix_out, float* campos_out, void* stream) {
  if (lr_pose_args(views, index, table, viewmatrix, projmatrix)) return LOGRAST_ERR_ARG;
  if (!viewmatrix_out || !projmatrix_out || !campos_out) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_pose_apply(table, index, viewmatrix, projmatrix, viewmatrix_out, projmatrix_out, campos_out, (hipStream_t)stream));
  return LOGRAST_OK;
}
int lograst_pose_backward(int32_t views, int32_t index, const float* table, const float* viewmatrix, const float* projmatrix,
                          const float* dl_dviewmatrix, const float* dl_dprojmatrix, const float* dl_dcampos, float* table_grad,
                          void* stream) {
  if (lr_pose_args(views, index, table, viewmatrix, projmatrix)) return LOGRAST_ERR_ARG;
  if (!table_grad) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (!dl_dviewmatrix && !dl_dprojmatrix && !dl_dcampos) return LOGRAST_OK;   // no gradient arrived: nothing to add
  g_prof_call++;
  LR_HIP(lr_launch_pose_backward(table, index, viewmatrix, projmatrix, dl_dviewmatrix, dl_dprojmatrix, dl_dcampos, table_grad,
                                 (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- densification (densify.hip) ---------------------------------------------------------------------------
static int lr_densify_children(int32_t children) {
  if (children != 2 && children != 4 && children != 8) return lr_fail(LOGRAST_ERR_ARG, "children must be 2, 4 or 8");
  return LOGRAST_OK;
}

size_t lograst_densify_scratch_bytes(int32_t p) { return lr_densify_scratch_bytes(p); }

int lograst_densify_plan(int32_t p, const uint8_t* flag_split, const uint8_t* flag_remove, int32_t remove_split,
                         int32_t children, const int32_t* node_index, const int32_t* index_parent, const int8_t* depth,
                         int32_t max_level, uint8_t* split_out, uint8_t* remove_out, int32_t* keep_dest, void* scratch,
                         size_t scratch_bytes, void* stream) {
  if (p < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (lr_densify_children(children)) return LOGRAST_ERR_ARG;
  if (!scratch || scratch_bytes < lr_densify_scratch_bytes(p)) return lr_fail(LOGRAST_ERR_ARG, "densify scratch too small");
  if (p > 0 && (!flag_split || !flag_remove || !split_out || !remove_out || !keep_dest)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if ((node_index != nullptr) != (index_parent != nullptr) || (node_index != nullptr) != (depth != nullptr))
    return lr_fail(LOGRAST_ERR_ARG, "node_index, index_parent and depth go together");
  if (p > 0 && (split_out == flag_split || remove_out == flag_remove)) return lr_fail(LOGRAST_ERR_ARG, "masked flags need their own storage");
  g_prof_call++;
  LR_HIP(lr_launch_densify_plan(p, flag_split, flag_remove, remove_split, node_index, index_parent, depth, max_level,
                                split_out, remove_out, keep_dest, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_densify_read(const void* scratch, uint32_t* num_keep_host, uint32_t* num_split_host, uint32_t* overlap_host,
                         void* stream) {
  if (!scratch) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  uint32_t w[3];
  LR_HIP(hipMemcpyAsync(w, scratch, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (num_keep_host) *num_keep_host = w[0];
  if (num_split_host) *num_split_host = w[1];
  if (overlap_host) *overlap_host = w[2];
  return LOGRAST_OK;
}

static int lr_densify_sizes(int32_t num_keep, int32_t num_split, int32_t children) {
  if (num_keep < 0 || num_split < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (lr_densify_children(children)) return LOGRAST_ERR_ARG;
  if ((int64_t)num_keep + (int64_t)num_split * children > (int64_t)0x7fffffff) return lr_fail(LOGRAST_ERR_ARG, "more than 2^31 - 1 new rows");
  return LOGRAST_OK;
}

int lograst_densify_src_rows(int32_t p, int32_t children, int32_t remove_split, const uint8_t* split, const uint8_t* remove,
                             int32_t num_keep, int32_t num_split, int32_t* src_row, const void* scratch, void* stream) {
  if (p < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (lr_densify_sizes(num_keep, num_split, children)) return LOGRAST_ERR_ARG;
  if (num_keep > p || num_split > p) return lr_fail(LOGRAST_ERR_ARG, "more kept or split rows than rows");
  if (num_keep + num_split == 0) return LOGRAST_OK;
  if (!split || !remove || !src_row || !scratch) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_densify_src_rows(p, children, remove_split, split, remove, num_keep, num_split, src_row, scratch,
                                    (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_densify_move_rows(int32_t num_keep, int32_t num_new, int32_t src_rows, const int32_t* src_row,
                              int32_t num_keys, const lograst_move_key* keys, void* stream) {
  if (num_keep < 0 || num_new < 0 || src_rows < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (num_keep > num_new) return lr_fail(LOGRAST_ERR_ARG, "num_keep exceeds num_new");
  if (num_keys < 0 || num_keys > LR_MOVE_MAX_KEYS) return lr_fail(LOGRAST_ERR_ARG, "at most 8 keys per call");
  if (num_keys > 0 && !keys) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  MoveArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < num_keys; i++) {
    const lograst_move_key& k = keys[i];
    if (k.elem_size != 1 && k.elem_size != 2 && k.elem_size != 4) return lr_fail(LOGRAST_ERR_ARG, "element size must be 1, 2 or 4");
    if (k.columns < 1 || (int64_t)k.columns * k.elem_size > 65536) return lr_fail(LOGRAST_ERR_ARG, "row size must be 1..65536 bytes");
    if (k.child_mode < LR_MOVE_COPY_PARENT || k.child_mode > LR_MOVE_SKIP) return lr_fail(LOGRAST_ERR_ARG, "unknown child mode");
    if (num_new > 0 && (!k.src || !k.dst)) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer in key");
    const uintptr_t sp = (uintptr_t)k.src, dp = (uintptr_t)k.dst;
    if ((dp & 15u) || (sp & (uintptr_t)(k.elem_size - 1))) return lr_fail(LOGRAST_ERR_ARG, "dst must be 16-byte aligned, src aligned to its element");
    const uint32_t rb = (uint32_t)k.columns * (uint32_t)k.elem_size;
    a.key[i].src = k.src; a.key[i].dst = k.dst; a.key[i].row_bytes = rb; a.key[i].child_mode = k.child_mode;
    a.key[i].unit = (rb % 4u == 0 && (sp & 3u) == 0) ? 4 : ((rb % 2u == 0 && (sp & 1u) == 0) ? 2 : 1);
    a.key[i].vec16 = (rb % 16u == 0 && (sp & 15u) == 0) ? 1 : 0;
  }
  if (num_new == 0 || num_keys == 0) return LOGRAST_OK;
  if (!src_row) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  a.src_row = src_row; a.num_keep = num_keep; a.num_new = num_new; a.src_rows = src_rows;
  g_prof_call++;
  LR_HIP(lr_launch_move_rows(a, num_keys, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_densify_split_uniform(int32_t num_keep, int32_t num_split, int32_t children, float scaling_factor,
                                  int32_t src_rows, const int32_t* src_row, const float* xyz, const float* scaling,
                                  const float* rotation, float* xyz_new, float* scaling_new, void* stream) {
  if (src_rows < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (lr_densify_sizes(num_keep, num_split, children)) return LOGRAST_ERR_ARG;
  if (num_split == 0) return LOGRAST_OK;
  if (!src_row || !xyz || !scaling || !rotation || !xyz_new || !scaling_new) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_split_uniform(num_keep, num_split, children, scaling_factor, src_rows, src_row, xyz, scaling, rotation,
                                 xyz_new, scaling_new, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_densify_tree(int32_t p, int32_t num_nodes, int32_t children, int32_t num_keep, int32_t num_split,
                         const int32_t* src_row, const int32_t* keep_dest, const uint8_t* split, const int32_t* node_index,
                         const int32_t* index_parent, const int8_t* local_index, const int8_t* depth, const int32_t* tree,
                         int32_t* node_index_new, int32_t* index_parent_new, int8_t* local_index_new, int8_t* depth_new,
                         int32_t* tree_new, void* stream) {
  if (p < 0 || num_nodes < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (lr_densify_sizes(num_keep, num_split, children)) return LOGRAST_ERR_ARG;
  if (num_keep > p || num_split > p) return lr_fail(LOGRAST_ERR_ARG, "more kept or split rows than rows");
  if (((int64_t)num_nodes + num_split) * children > (int64_t)0x7fffffff) return lr_fail(LOGRAST_ERR_ARG, "tree too large");
  const int64_t num_new = (int64_t)num_keep + (int64_t)num_split * children;
  if (num_new > 0 && (!src_row || !keep_dest || !split || !node_index || !index_parent || !local_index || !depth ||
                      !node_index_new || !index_parent_new || !local_index_new || !depth_new))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if ((num_nodes > 0 && (!tree || !keep_dest)) || (num_nodes + num_split > 0 && !tree_new)) return lr_fail(LOGRAST_ERR_ARG, "NULL tree pointer");
  TreeArgs a;
  a.src_row = src_row; a.keep_dest = keep_dest; a.split = split;
  a.node_index = node_index; a.index_parent = index_parent; a.local_index = local_index; a.depth = depth; a.tree = tree;
  a.node_index_new = node_index_new; a.index_parent_new = index_parent_new; a.local_index_new = local_index_new;
  a.depth_new = depth_new; a.tree_new = tree_new;
  a.p = p; a.num_nodes = num_nodes; a.children = children; a.num_keep = num_keep; a.num_split = num_split;
  g_prof_call++;
  LR_HIP(lr_launch_densify_tree(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- densification decisions (decide.hip) ------------------------------------------------------------------
size_t lograst_decide_scratch_bytes(int32_t p) { return lr_decide_scratch_bytes(p); }

static int lr_decide_common(int32_t p, const void* args, const void* scratch, size_t scratch_bytes) {
  if (p < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (!args) return lr_fail(LOGRAST_ERR_ARG, "args is NULL");
  if (!scratch || scratch_bytes < lr_decide_scratch_bytes(p)) return lr_fail(LOGRAST_ERR_ARG, "decide scratch too small");
  if (reinterpret_cast<uintptr_t>(scratch) & 15u) return lr_fail(LOGRAST_ERR_ARG, "decide scratch must be 16-byte aligned");
  return LOGRAST_OK;
}

int lograst_decide_depth(int32_t p, const lograst_decide_depth_args* args, void* scratch, size_t scratch_bytes, void* stream) {
  if (lr_decide_common(p, args, scratch, scratch_bytes)) return LOGRAST_ERR_ARG;
  const lograst_decide_depth_args& a = *args;
  if (p > 0 && (!a.opacity || !a.scaling || !a.node_index || !a.depth || !a.create_steps || !a.grad_sum || !a.area_sum ||
                !a.radii_max_max || !a.weights_max || !a.visible_count || !a.flag_split || !a.flag_remove))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (p > 0 && a.flag_split == a.flag_remove) return lr_fail(LOGRAST_ERR_ARG, "flag_split and flag_remove need their own storage");
  if (a.current_depth < -128 || a.current_depth > 128 || a.max_level < -128 || a.max_level > 128)
    return lr_fail(LOGRAST_ERR_ARG, "current_depth / max_level outside -128..128 (depth is int8: clip them)");
  g_prof_call++;
  LR_HIP(lr_launch_decide_depth(p, a, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_decide_init(int32_t p, const lograst_decide_init_args* args, void* scratch, size_t scratch_bytes, void* stream) {
  if (lr_decide_common(p, args, scratch, scratch_bytes)) return LOGRAST_ERR_ARG;
  const lograst_decide_init_args& a = *args;
  if (p > 0 && (!a.opacity || !a.create_steps || !a.grad_sum || !a.area_sum || !a.radii_max_max || !a.weights_max ||
                !a.rand || !a.radius3d_min || !a.flag_split || !a.flag_remove))
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (p > 0 && a.flag_split == a.flag_remove) return lr_fail(LOGRAST_ERR_ARG, "flag_split and flag_remove need their own storage");
  if (a.children < 1 || a.children > 8) return lr_fail(LOGRAST_ERR_ARG, "children must be 1..8");
  g_prof_call++;
  LR_HIP(lr_launch_decide_init(p, a, scratch, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_decide_read(const void* scratch, lograst_decide_record* record_host, size_t record_bytes, void* stream) {
  if (!scratch || !record_host) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (record_bytes != sizeof(lograst_decide_record)) return lr_fail(LOGRAST_ERR_ARG, "record_bytes is not sizeof(lograst_decide_record)");
  LR_HIP(hipMemcpyAsync(record_host, scratch, sizeof(lograst_decide_record), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_decide_child_radius_max(int32_t num_points, int32_t num_children, const int32_t* index_parent,
                                    const float* scaling, float scaling_decay, float* radius3d_max, void* stream) {
  if (num_points < 0 || num_children < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (num_children > num_points) return lr_fail(LOGRAST_ERR_ARG, "more children than rows");
  if (num_children == 0) return LOGRAST_OK;
  if (!index_parent || !scaling || !radius3d_max) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  g_prof_call++;
  LR_HIP(lr_launch_child_radius_max(num_points, num_children, index_parent, scaling, scaling_decay, radius3d_max,
                                    (hipStream_t)stream));
  return LOGRAST_OK;
}

static int lr_ga_check(int32_t n, int32_t sh_coeffs, int32_t active_degree, const float* camera_center) {
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative row count");
  if (sh_coeffs < 0 || sh_coeffs > 15) return lr_fail(LOGRAST_ERR_ARG, "sh_coeffs must be 0..15 (degree <= 3)");
  if (active_degree < 0 || active_degree > 3) return lr_fail(LOGRAST_ERR_ARG, "active SH degree must be 0..3");
  if (active_degree > 0 && (active_degree + 1) * (active_degree + 1) - 1 > sh_coeffs)
    return lr_fail(LOGRAST_ERR_ARG, "shs holds fewer coefficients than the active degree needs");
  if (active_degree > 0 && !camera_center) return lr_fail(LOGRAST_ERR_ARG, "camera_center is NULL");
  return LOGRAST_OK;
}
// the quaternion blocks are read and written as float4 (the third pointer may be absent)
static bool lr_aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}
// The front of the three lograst_activate_backward*: lr_ga_check, then -- unless n == 0, which the caller returns as OK -- the
// model's size where the call has one (`num_points`; the plain backward passes 1), the NULL check of the common pointers
// together with the caller's own (`others`: all of them non-NULL), the alignment of the quaternion blocks (`rotation_out`
// is the plain backward's third) under the caller's message, and the inputs of ActBwdArgs; the outputs stay NULL.
static int lr_act_bwd_args(ActBwdArgs& a, int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                           const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree, const float* camera_center,
                           const float* dl_dact_scaling, const float* dl_dact_opacity, const float* dl_dact_rotation,
                           const float* dl_dact_colors, int32_t num_points, bool others, const float* rotation_out,
                           const char* alignment) {
  int rc = lr_ga_check(n, sh_coeffs, active_degree, camera_center);
  if (rc || n == 0) return rc;
  if (num_points <= 0) return lr_fail(LOGRAST_ERR_ARG, "rows of an empty model");
  if (!raw_xyz || !raw_scaling || !raw_opacity || !raw_rotation || !dl_dact_scaling || !dl_dact_opacity || !dl_dact_rotation ||
      !dl_dact_colors || !others)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (!lr_aligned16(raw_rotation, dl_dact_rotation, rotation_out)) return lr_fail(LOGRAST_ERR_ARG, alignment);
  memset(&a, 0, sizeof(a));
  a.r_xyz = raw_xyz; a.r_scaling = raw_scaling; a.r_opacity = raw_opacity; a.r_rotation = raw_rotation;
  a.campos = camera_center;
  a.g_a_scaling = dl_dact_scaling; a.g_a_opacity = dl_dact_opacity; a.g_a_rotation = dl_dact_rotation;
  a.g_a_colors = dl_dact_colors;
  a.n = n; a.K = sh_coeffs; a.deg = active_degree;
  return LOGRAST_OK;
}
static const char kAlignStep[] = "raw_rotation / dl_dact_rotation must be 16-byte aligned";

int lograst_gather_activate(int32_t n, int32_t num_points, const int64_t* index, const float* xyz,
                            const float* scaling, const float* opacity, const float* rotation, const float* colors,
                            const float* shs, int32_t sh_coeffs, int32_t active_degree, const float* camera_center,
                            float* raw_xyz, float* raw_scaling, float* raw_opacity, float* raw_rotation,
                            float* raw_colors, float* raw_shs, float* act_scaling, float* act_opacity,
                            float* act_rotation, float* act_colors, void* stream) {
  int rc = lr_ga_check(n, sh_coeffs, active_degree, camera_center);
  if (rc) return rc;
  if (n == 0) return LOGRAST_OK;
  if (num_points <= 0) return lr_fail(LOGRAST_ERR_ARG, "rows requested from an empty model");
  if (!index || !xyz || !scaling || !opacity || !rotation || !colors || !raw_xyz || !raw_scaling || !raw_opacity ||
      !raw_rotation || !raw_colors || !act_scaling || !act_opacity || !act_rotation || !act_colors)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  if (sh_coeffs > 0 && (!shs || !raw_shs)) return lr_fail(LOGRAST_ERR_ARG, "NULL shs pointer");
  if (!lr_aligned16(rotation, raw_rotation, act_rotation))
    return lr_fail(LOGRAST_ERR_ARG, "rotation / raw_rotation / act_rotation must be 16-byte aligned");
  GatherArgs a;
  a.index = index; a.xyz = xyz; a.scaling = scaling; a.opacity = opacity; a.rotation = rotation; a.colors = colors;
  a.shs = shs; a.campos = camera_center;
  a.r_xyz = raw_xyz; a.r_scaling = raw_scaling; a.r_opacity = raw_opacity; a.r_rotation = raw_rotation;
  a.r_colors = raw_colors; a.r_shs = raw_shs;
  a.a_scaling = act_scaling; a.a_opacity = act_opacity; a.a_rotation = act_rotation; a.a_colors = act_colors;
  a.n = n; a.num_points = num_points; a.K = sh_coeffs; a.deg = active_degree;
  g_prof_call++;
  LR_HIP(lr_launch_gather_activate(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_activate_backward(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                              const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                              const float* camera_center, const float* dl_dact_scaling, const float* dl_dact_opacity,
                              const float* dl_dact_rotation, const float* dl_dact_colors, float* dl_dscaling,
                              float* dl_dopacity, float* dl_drotation, float* dl_dcolors, float* dl_dshs, void* stream) {
  ActBwdArgs a;
  int rc = lr_act_bwd_args(a, n, raw_xyz, raw_scaling, raw_opacity, raw_rotation, sh_coeffs, active_degree, camera_center,
                           dl_dact_scaling, dl_dact_opacity, dl_dact_rotation, dl_dact_colors, 1,
                           dl_dscaling && dl_dopacity && dl_drotation && dl_dcolors, dl_drotation,
                           "raw_rotation / dl_dact_rotation / dl_drotation must be 16-byte aligned");
  if (rc || n == 0) return rc;
  a.g_scaling = dl_dscaling; a.g_opacity = dl_dopacity; a.g_rotation = dl_drotation; a.g_colors = dl_dcolors;
  a.g_shs = dl_dshs;
  g_prof_call++;
  LR_HIP(lr_launch_activate_bwd(a, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_activate_backward_adam(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                                   const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                                   const float* camera_center, const float* dl_dact_xyz, const float* dl_dact_scaling,
                                   const float* dl_dact_opacity, const float* dl_dact_rotation, const float* dl_dact_colors,
                                   int32_t num_points, const int64_t* index, const int32_t* radii,
                                   const lograst_adam_key* keys, double beta1, double beta2, double bias_correction2_sqrt,
                                   double eps, void* stream) {
  ActBwdArgs a;
  int rc = lr_act_bwd_args(a, n, raw_xyz, raw_scaling, raw_opacity, raw_rotation, sh_coeffs, active_degree, camera_center,
                           dl_dact_scaling, dl_dact_opacity, dl_dact_rotation, dl_dact_colors, num_points,
                           dl_dact_xyz && index && radii && keys, nullptr, kAlignStep);
  if (rc || n == 0) return rc;
  AdamArgs f;
  memset(&f, 0, sizeof(f));
  for (int i = 0; i < 6; i++) {
    const lograst_adam_key& k = keys[i];
    if (!k.model_param) continue;                            // key not optimised in this step
    if (k.width != lr_step_key_width(i, sh_coeffs)) return lr_fail(LOGRAST_ERR_ARG, "lograst_activate_backward_adam: key widths are 3, 3, 1, 4, 3, 3 * sh_coeffs (xyz, scaling, opacity, rotation, colors, shs)");
    if (i == 5 && (sh_coeffs == 0 || active_degree == 0)) return lr_fail(LOGRAST_ERR_ARG, "shs key without active SH coefficients");
    if ((rc = lr_adam_key(f.key[i], k, true, false))) return rc;
  }
  f.index = index; f.flag_vis = nullptr; f.m = n; f.num_points = num_points;
  lr_adam_scalars(f, beta1, beta2, bias_correction2_sqrt, eps);
  g_prof_call++;
  LR_HIP(lr_launch_activate_bwd_adam(a, f, dl_dact_xyz, radii, (hipStream_t)stream));
  return LOGRAST_OK;
}

// ---- steps over several views (accumulate.hip) ----------------------------------------------------------------------------
size_t lograst_accumulate_target_floats(int32_t num_points, int32_t row_stride_floats, int32_t width) {
  if (num_points <= 0 || row_stride_floats < 0 || width < 0) return 0;
  return lr_acc_offset((int64_t)num_points - 1, row_stride_floats, width);
}

int lograst_activate_backward_accumulate(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                                         const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                                         const float* camera_center, const float* dl_dact_xyz, const float* dl_dact_scaling,
                                         const float* dl_dact_opacity, const float* dl_dact_rotation,
                                         const float* dl_dact_colors, int32_t num_points, const int64_t* index,
                                         const int32_t* radii, const lograst_acc_target* targets, int32_t* seen,
                                         void* stream) {
  ActBwdArgs a;
  int rc = lr_act_bwd_args(a, n, raw_xyz, raw_scaling, raw_opacity, raw_rotation, sh_coeffs, active_degree, camera_center,
                           dl_dact_scaling, dl_dact_opacity, dl_dact_rotation, dl_dact_colors, num_points,
                           dl_dact_xyz && index && radii && targets && seen, nullptr, kAlignStep);
  if (rc || n == 0) return rc;
  AccArgs t;
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < ACC_KEYS; i++) {
    if (!targets[i].base) continue;
    if (i == 5 && sh_coeffs == 0) return lr_fail(LOGRAST_ERR_ARG, "shs target without SH coefficients");
    if (targets[i].row_stride_floats < lr_step_key_width(i, sh_coeffs))
      return lr_fail(LOGRAST_ERR_ARG, "lograst_activate_backward_accumulate: a target's row stride is smaller than its key's width (3, 3, 1, 4, 3, 3 * sh_coeffs)");
    t.t[i].base = targets[i].base; t.t[i].stride = targets[i].row_stride_floats;
  }
  t.g_a_xyz = dl_dact_xyz; t.index = index; t.radii = radii; t.seen = seen; t.num_points = num_points;
  g_prof_call++;
  LR_HIP(lr_launch_activate_bwd_accumulate(a, t, (hipStream_t)stream));
  return LOGRAST_OK;
}

int lograst_accumulated_adam(int32_t num_points, int32_t* seen, const lograst_adam_key* keys,
                             const int32_t* grad_row_stride_floats, double beta1, double beta2,
                             double bias_correction2_sqrt, double eps, uint8_t* moved_out, void* stream) {
  if (num_points < 0) return lr_fail(LOGRAST_ERR_ARG, "negative count");
  if (num_points == 0) return LOGRAST_OK;
  if (!seen || !keys || !grad_row_stride_floats) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  AdamArgs f;
  memset(&f, 0, sizeof(f));
  AccStepArgs t;
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < ACC_KEYS; i++) {
    const lograst_adam_key& k = keys[i];
    if (!k.model_param) continue;                            // key not optimised
    // (no sh_coeffs in this call: the shs key is as wide as some count of 1..15 coefficients makes it)
    if (i == 5 ? (k.width < 3 || k.width > 45 || k.width % 3) : k.width != lr_step_key_width(i, 0))
      return lr_fail(LOGRAST_ERR_ARG, "lograst_accumulated_adam: key widths are 3, 3, 1, 4, 3, 3 * sh_coeffs (xyz, scaling, opacity, rotation, colors, shs)");
    int rc = lr_adam_key(f.key[i], k, false, true);
    if (rc) return rc;
    if (grad_row_stride_floats[i] < k.width) return lr_fail(LOGRAST_ERR_ARG, "lograst_accumulated_adam: a gradient row stride is smaller than its key's width");
    t.gstride[i] = grad_row_stride_floats[i];
  }
  f.num_points = num_points;
  lr_adam_scalars(f, beta1, beta2, bias_correction2_sqrt, eps);
  t.seen = seen; t.moved = moved_out;
  g_prof_call++;
  LR_HIP(lr_launch_accumulated_adam(f, t, (hipStream_t)stream));
  return LOGRAST_OK;
}

static int lr_sh_check(int32_t n, int32_t degree, int32_t max_coeffs) {
  if (n < 0) return lr_fail(LOGRAST_ERR_ARG, "negative Gaussian count");
  if (degree < 0 || degree > 3) return lr_fail(LOGRAST_ERR_ARG, "SH degree must be 0..3");
  if (max_coeffs < (degree + 1) * (degree + 1) || max_coeffs > 16)
    return lr_fail(LOGRAST_ERR_ARG, "shs must hold (degree+1)^2 .. 16 coefficients per Gaussian");
  return LOGRAST_OK;
}

int lograst_sh_forward(int32_t n, int32_t degree, int32_t max_coeffs, const float* means3d, const float* campos,
                       const float* shs, float* colors, uint8_t* clamped, void* stream) {
  int rc = lr_sh_check(n, degree, max_coeffs);
  if (rc) return rc;
  if (n == 0) return LOGRAST_OK;
  if (!means3d || !campos || !shs || !colors || !clamped) return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  lr_launch_sh_fwd(n, degree, max_coeffs, means3d, campos, shs, colors, clamped, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

int lograst_sh_backward(int32_t n, int32_t degree, int32_t max_coeffs, const float* means3d, const float* campos,
                        const float* shs, const uint8_t* clamped, const float* dl_dcolors, float* dl_dshs,
                        float* dl_dmeans3d, int32_t accumulate, void* stream) {
  int rc = lr_sh_check(n, degree, max_coeffs);
  if (rc) return rc;
  if (n == 0) return LOGRAST_OK;
  if (!means3d || !campos || !shs || !clamped || !dl_dcolors || !dl_dshs || !dl_dmeans3d)
    return lr_fail(LOGRAST_ERR_ARG, "NULL pointer");
  lr_launch_sh_bwd(n, degree, max_coeffs, means3d, campos, shs, clamped, dl_dcolors, dl_dshs, dl_dmeans3d,
                   accumulate != 0, (hipStream_t)stream);
  LR_HIP(hipGetLastError());
  return LOGRAST_OK;
}

void lograst_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
}
void lograst_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  lr_prof_drain_locked();
  std::memset(g_prof_ms, 0, sizeof(g_prof_ms));
  std::memset(g_prof_cnt, 0, sizeof(g_prof_cnt));
}
int lograst_profile_read(double* ms_out, int64_t* count_out) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  lr_prof_drain_locked();
  for (int i = 0; i < LOGRAST_NUM_KERNELS; i++) {
    if (ms_out) ms_out[i] = g_prof_ms[i];
    if (count_out) count_out[i] = g_prof_cnt[i];
  }
  return LOGRAST_OK;
}
const char* lograst_kernel_name(int slot) {
  return (slot >= 0 && slot < LOGRAST_NUM_KERNELS) ? kKernelNames[slot] : "";
}

}  // extern "C"
