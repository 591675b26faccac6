// launch.hpp -- the host-side launchers and sizing helpers that the kernel files define and api.hip calls, declared once:
// api.hip and every defining .hip file include this header, so a definition that drifts from its prototype does not compile.
#pragma once
#include "common.hpp"

// project.hip
void lr_launch_radius(int P, const float* means, const float* scales, const float* rots, const float* proj,
                      const float* view, float fx, float fy, float tanfovx, float tanfovy, float* radii,
                      hipStream_t s);
bool lr_band_sparse(const LrView& v, int batch);
// band: lr_band_sparse(v, batch), as the caller's plan holds it
void lr_launch_project(const LrView& v, int N, const float* means, const float* scales, const float* rots,
                       const float* opac, const float* colors, int* radii, void* geom, uint32_t* ranked,
                       uint32_t* big, uint32_t* hdr, uint32_t* basetab, int batch, int planes, bool band, int tile_cull,
                       hipStream_t s);
void lr_launch_scan(uint32_t* state, uint32_t tiles, uint32_t cs, uint32_t big_off, hipStream_t s);
void lr_launch_rebase(uint32_t* state, uint32_t tiles, uint32_t batches, uint32_t t_lo, uint32_t t_hi, hipStream_t s);
void lr_launch_zero_words(uint32_t* p, size_t words, hipStream_t s);
void lr_launch_zero_floats(float* p, size_t n, hipStream_t s);
void lr_launch_fill(int N, int gx, const void* geom, uint32_t* state, uint32_t tiles, uint64_t* keys,
                    uint32_t capacity, uint32_t max_len_hint, uint32_t* status, float* zero_n, float* zero_block,
                    int zero_block_floats, int rebased, int speculative, int band, int staged_k, hipStream_t s);
void lr_launch_tile_rows(const LrView& v, int N, const float* means, const float* scales, const float* rots,
                         uint32_t* rows, hipStream_t s);
void lr_launch_stream_copy(const void* src, void* dst, size_t bytes, int blocks, hipStream_t s);
// lograst_recomposite: records = geom's N 64-byte records with the colour fields taken from colors[N, 3] (radii > 0 only),
// radii_out = radii, zero_n[N] (or NULL) and zero_rows[N][16] (or NULL) cleared, the pass recorded in status (or NULL)
void lr_launch_recolor(int N, const int* radii, const void* geom, const float* colors, void* records, int* radii_out,
                       float* zero_n, float* zero_rows, const uint32_t* state, uint32_t* status, hipStream_t s);

// sort.hip
void lr_launch_sort(uint32_t* state, uint32_t tiles, uint64_t* keys, uint32_t* plist, uint32_t capacity,
                    uint32_t max_len, int lazy, hipStream_t s);
void lr_launch_sort_rest(uint32_t* state, uint32_t tiles, uint64_t* keys, uint32_t* plist, uint32_t capacity,
                         uint32_t max_len, int mode, hipStream_t s);
void lr_launch_ordered_lengths(const uint32_t* state, uint32_t tiles, uint32_t* out, hipStream_t s);

// blend.hip
// The launchers' arguments as records: a call site names every field it sets, and the ones it leaves out are NULL / 0 = off.
struct LrBlendFwdArgs {
  const void* geom; const uint32_t* state; uint32_t tiles; const uint32_t* plist; uint32_t capacity;
  float *image, *final_T; int *n_contrib, *pid; float *pwp, *pw;
  float* zero_conic;            // the accumulator rows the kernel clears as it meets them, or NULL
  int big_input, lazy; uint64_t* masks;
  const float* aux_colors; float* aux_image;   // aux: quadrant form, whatever the view says
};
void lr_launch_blend_fwd(const LrView& v, const LrBlendFwdArgs& a, hipStream_t s);
int lr_blend_fwd_form(const LrView& v);
int lr_blend_bwd_form(const LrView& v, int big_input);
struct LrBlendBwdArgs {
  const void* geom; const uint32_t* state; uint32_t tiles; const uint32_t* plist; uint32_t capacity;
  const float* final_T; const int* n_contrib; const float* dL_dimage; float* acc_rows; int big_input; const uint64_t* masks;
  const float *aux_colors, *dL_daux;   // aux: quadrant form; either gradient may be NULL
  bool abs_sums;                       // (no aux): |per-pixel terms of dL/dmean x, y| summed into the rows' slots 9, 10
};
void lr_launch_blend_bwd(const LrView& v, const LrBlendBwdArgs& a, hipStream_t s);

// project_bwd.hip
struct LrProjectBwdArgs {
  int N; const float *means, *scales, *rots; const int* radii;
  const float *g_mean2d, *g_conic;   // lograst_project_backward's inputs, or
  const float* rows;                 // the 64-byte accumulator rows of lograst_backward (+ its three separate outputs)
  float *o_mean2d, *o_opac, *o_col; const float* pw;
  float *g_means3d, *g_scales, *g_rots;
  bool accumulate, sink_rows;
  bool big_input;                    // the caller's large-input predicate (n >= LOGRAST_HELPER_MIN_N); only looked at with rows
  float* o_aux;                      // dL/daux_colors [N, 3] out of the rows' slots 9..11 (fresh gradients, no cov3d)
  float *cam_partials, *cam_dv, *cam_dp;   // the camera sums (below; fresh gradients, no cov3d, no o_aux)
  float* o_abs;                      // dl_dmeans2d_abs [N, 3] out of the rows' slots 9, 10 (fresh gradients, no cov3d, no o_aux, no camera sums)
};
void lr_launch_project_bwd(const LrView& v, const LrProjectBwdArgs& a, hipStream_t s);

// cam_partials (+ cam_dv, cam_dp [4, 4]): the camera sums -- one row of 24 partials per workgroup of the chain rule, then
// dL/dviewmatrix / dL/dprojmatrix by a finishing kernel; lr_camera_scratch_bytes(N) bytes (fresh gradients, no cov3d, no o_aux)
size_t lr_camera_scratch_bytes(int N);

// exchange.hip
void lx_launch_pack_rows(float* rows, int groups, long long rows_per_group, int kmax, float* packed,
                         size_t seg_floats, uint32_t* overflow, int clear, const uint32_t* hint, long long hint_rows,
                         hipStream_t s);
void lx_launch_add_visible(float* seen, const int32_t* radii, long long n, hipStream_t s);
void lx_launch_add_visible_n(float* seen, const int32_t* const* radii, int k, long long n, hipStream_t s);
void lx_launch_unpack_rows(float* dest, const float* packed, int segments, int kmax, size_t seg_floats,
                           long long rows_per_group, long long dest_group_rows, int add, int zero, hipStream_t s);

// knn.hip
size_t lr_knn_scratch_bytes(int P);
hipError_t lr_launch_knn(int P, const float* pts, float* out, void* scratch, size_t scratch_bytes, hipStream_t s);

// sh.hip
void lr_launch_sh_fwd(int N, int deg, int M, const float* means, const float* campos, const float* shs, float* colors,
                      uint8_t* clamped, hipStream_t s);
void lr_launch_sh_bwd(int N, int deg, int M, const float* means, const float* campos, const float* shs,
                      const uint8_t* clamped, const float* g_colors, float* g_shs, float* g_means, bool accumulate,
                      hipStream_t s);
hipError_t lr_launch_gather_activate(const GatherArgs& a, hipStream_t s);
hipError_t lr_launch_activate_bwd(const ActBwdArgs& a, hipStream_t s);
hipError_t lr_launch_activate_bwd_adam(const ActBwdArgs& a, const AdamArgs& f, const float* g_a_xyz, const int32_t* radii,
                                       hipStream_t s);

// accumulate.hip
hipError_t lr_launch_activate_bwd_accumulate(const ActBwdArgs& a, const AccArgs& t, hipStream_t s);
hipError_t lr_launch_accumulated_adam(const AdamArgs& f, const AccStepArgs& t, hipStream_t s);

// lod.hip
size_t lr_lod_scratch_bytes(int num_roots, int num_nodes, int max_child);
hipError_t lr_launch_lod(int num_points, int num_nodes, int max_child, const int32_t* node_index, const int32_t* tree,
                         const float* xyz, const float* scaling, const float* rotation, const int64_t* root_index,
                         int num_roots, const float* proj, const float* view, float fx, float fy, float tanfovx,
                         float tanfovy, float min_px, int levels, int64_t* out, uint32_t out_capacity, void* scratch,
                         hipStream_t s);
int lr_lod_max_levels();
uint32_t lr_lod_total_word();   // header words TOTAL, OVERFLOW, LEFT are consecutive; the next one is cleared by every
                                // traversal and otherwise unused by lod.hip: lograst_lod_select keeps the leaf count there

// prepare.hip
size_t lr_frustum_scratch_bytes(int n);   // word 0: the kept count
// rows == NULL: entry i is row i; scaling == NULL: no activated outputs (then rotation, opacity and the four o_* are NULL too)
hipError_t lr_launch_frustum(int n, int num_points, const float* xyz, const int32_t* rows, const float* proj, float lo,
                             float hi, const float* scaling, const float* rotation, const float* opacity, uint8_t* flag,
                             int64_t* pos, int64_t* row_out, float* o_xyz, float* o_scaling, float* o_rotation,
                             float* o_opacity, void* scratch, hipStream_t s);
hipError_t lr_launch_root_filter(int k_roots, const int64_t* rows, const float* weight, const int64_t* pos,
                                 uint8_t* root_flag, int num_flags, int64_t* rows_out, hipStream_t s);
size_t lr_partition_scratch_bytes(uint32_t capacity);
// n_dev: the list's length, on the device (capped at capacity); leaf_total: where the number of leaves goes
hipError_t lr_launch_partition(const int64_t* list, const uint32_t* n_dev, uint32_t capacity, const int32_t* node_index,
                               const int8_t* depth, int num_points, int all_levels, int current_depth, int64_t* out_leaf,
                               int64_t* out_node, uint32_t* chunk, uint32_t* leaf_total, hipStream_t s);
hipError_t lr_launch_clamp_scale(int m, const int64_t* index, const uint8_t* flag, int num_points, float* scaling,
                                 const float* rmin, const float* rmax, hipStream_t s);

// init.hip
// cameras: V x 36 floats on the device (proj[16], view[16], fx, fy, tanfovx, tanfovy); radius3d_min in/out or NULL;
// valid / radius3d: NULL unless V == 1
hipError_t lr_launch_init_radius3d(int P, const float* xyz, const float* scaling, const float* rotation, int V,
                                   const float* cameras, float* radius3d_min, uint8_t* valid, float* radius3d,
                                   hipStream_t s);

// counter.hip
size_t lr_hist_scratch_bytes(int n);
hipError_t lr_launch_id_histogram(int n, const int32_t* pid, int npix, int32_t* ids, int64_t* counts, void* scratch,
                                  hipStream_t s);
hipError_t lr_launch_counter(const CounterArgs& a, hipStream_t s);
hipError_t lr_launch_sparse_adam(const AdamArgs& a, int num_keys, hipStream_t s);
hipError_t lr_launch_corrector_step(const CorrectorArgs& a, hipStream_t s);

// pose.hip: one row of a [views, 6] pose table applied to a camera, and dL/d(row) added into the table's gradient
hipError_t lr_launch_pose_apply(const float* table, int index, const float* view, const float* proj, float* view_out,
                                float* proj_out, float* campos_out, hipStream_t s);
hipError_t lr_launch_pose_backward(const float* table, int index, const float* view, const float* proj, const float* g_view,
                                   const float* g_proj, const float* g_campos, float* grad, hipStream_t s);

// loss.hip
size_t lr_loss_scratch_bytes(int B, int C, int H, int W);
size_t lr_loss_gain_scratch_bytes(int B, int C, int H, int W);
// a.gain selects the GAIN instantiations (and the reduction into grad_gain); a.mask or a.fg the MASKED forward, a.mask the
// MASKED backward
hipError_t lr_launch_loss_fwd(const LossArgs& a, float wa, float wb, float* out3, hipStream_t s);
hipError_t lr_launch_loss_bwd(const LossArgs& a, const float* grad_loss, float* g_render, float* g_render_l1, float* grad_gain,
                              hipStream_t s);
#define MB_RECORD_INTS 8        // per image: xmin, ymin, xmax, ymax, count, 0, 0, 0
hipError_t lr_launch_mask_bounds(int B, int H, int W, const float* mask, const int64_t* ms, float threshold, int32_t* record, hipStream_t s);

// depth_loss.hip
#define DL_PATCH 64             // the patch side, the only one the kernels have
#define DL_MAX_PATCHES 256
#define DL_REC 16               // doubles per record slot: slot 0 the header, slot 1 + k patch k (layout: depth_loss.hip)
struct DepthLossArgs {
  const float* pred; const float* gt; const float* acc;   // [H, W] each
  int64_t ps[2], gs[2], as[2];                            // element strides (y, x)
  int32_t H, W;
};
size_t lr_depth_loss_record_bytes(int n);
hipError_t lr_launch_depth_loss_fwd(const DepthLossArgs& a, int n, const int64_t* rows, const int64_t* cols, double alpha,
                                    double eps, double thr, void* out, double* records, hipStream_t s);
hipError_t lr_launch_depth_loss_bwd(const DepthLossArgs& a, int n, const double* records, const float* grad_loss,
                                    float* grad_pred, hipStream_t s);

// evaluate.hip
struct EvalArgs {
  const float* pred; const float* gt;       // [C, H, W] each
  int64_t ps[3], gs[3];                     // element strides (c, y, x)
  int32_t C, H, W, ntx;
  float w[LS_WIN_TAPS];                     // the SSIM window (the loss's table)
  float c1, c2;                             // (0.01 max_val)^2, (0.03 max_val)^2
  float* corrected;                         // [C, H, W] contiguous, or NULL
  uint8_t* bgr8;                            // metrics: [2 H, W, C]; the export alone: [H, W, C]; or NULL
  double* record;                           // 16 doubles (layout: evaluate.hip)
  double* gain_partial; double* partial;    // inside the scratch
};
size_t lr_eval_scratch_bytes(int C, int H, int W);
hipError_t lr_launch_eval_bgr8(const EvalArgs& a, hipStream_t s);
hipError_t lr_launch_eval_metrics(EvalArgs a, bool fit_gain, bool ssim, void* scratch, hipStream_t s);

// densify.hip
#define LR_MOVE_COPY_PARENT 0   // rows >= num_keep copy src[src_row[d]] like the kept rows
#define LR_MOVE_ZERO 1          // rows >= num_keep are zero
#define LR_MOVE_SKIP 2          // rows >= num_keep are left to another kernel
#define LR_MOVE_MAX_KEYS 8
struct MoveKey {
  const void* src; void* dst;   // [src_rows, row_bytes] -> [num_new, row_bytes]; dst 16-byte aligned
  uint32_t row_bytes;
  int32_t unit;                 // 4 | 2 | 1: the largest access that every row start of src allows
  int32_t vec16;                // row_bytes % 16 == 0 and src 16-byte aligned
  int32_t child_mode;
};
struct MoveArgs {
  MoveKey key[LR_MOVE_MAX_KEYS];
  const int32_t* src_row;       // [num_new]
  int32_t num_keep, num_new, src_rows;
};
struct TreeArgs {
  const int32_t* src_row; const int32_t* keep_dest; const uint8_t* split;
  const int32_t* node_index; const int32_t* index_parent; const int8_t* local_index; const int8_t* depth;
  const int32_t* tree;          // [num_nodes, children]
  int32_t* node_index_new; int32_t* index_parent_new; int8_t* local_index_new; int8_t* depth_new;   // [num_new]
  int32_t* tree_new;            // [num_nodes + num_split, children]
  int32_t p, num_nodes, children, num_keep, num_split;
};
size_t lr_densify_scratch_bytes(int p);
hipError_t lr_launch_densify_plan(int p, const uint8_t* flag_split, const uint8_t* flag_remove, int remove_split,
                                  const int32_t* node_index, const int32_t* index_parent, const int8_t* depth,
                                  int max_level, uint8_t* split_out, uint8_t* remove_out, int32_t* keep_dest,
                                  void* scratch, hipStream_t s);
hipError_t lr_launch_densify_src_rows(int p, int children, int remove_split, const uint8_t* split, const uint8_t* remove,
                                      int num_keep, int num_split, int32_t* src_row, const void* scratch, hipStream_t s);
hipError_t lr_launch_move_rows(const MoveArgs& a, int num_keys, hipStream_t s);
hipError_t lr_launch_split_uniform(int num_keep, int num_split, int children, float factor, int src_rows,
                                   const int32_t* src_row, const float* xyz, const float* scaling, const float* rotation,
                                   float* xyz_new, float* scaling_new, hipStream_t s);
hipError_t lr_launch_densify_tree(const TreeArgs& a, hipStream_t s);
