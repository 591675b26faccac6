/*
 * lograst.h -- C ABI of liblograst.so: the MI355X (gfx950) differentiable Gaussian-splatting
 * rasterizer behind LoG's operator surface.
 *
 * The reference (zju3dv/LoG) has no C ABI of its own: its boundary is two pybind11 torch extensions
 * built from third-party repos plus one in-tree JIT extension.  Each entry point below
 * names the reference interface it stands behind; the Python shims that reproduce those interfaces
 * one-to-one live in log_amd/rasterizer.py and log_amd/compute_radius.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; all floats are fp32;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); nothing synchronises the
 *     host except lograst_forward_project when `num_instances_host` != NULL, and lograst_profile_read;
 *   - no allocation happens inside the library: the caller sizes scratch with the *_bytes helpers
 *     (the Python shim uses torch's caching allocator);
 *   - return value 0 = success, negative = error (lograst_last_error() gives the text);
 *   - matrices use LoG's row-vector convention, flat row-major: t = p_row @ M
 *     (/root/reference/LoG/dataset/base.py:40-46).
 */
#ifndef LOGRAST_H
#define LOGRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOGRAST_VERSION 4   /* 4 (round 6): contracts that changed since 3 -- (a) lograst_geom_bytes grew by 8 B per Gaussian + 256 KB (the
 * rank rows of the 5-16-tile rects behind the fill records and indices: a caller that sized `geom` as 84 B per Gaussian gets
 * out-of-bounds writes; always size it with lograst_geom_bytes); (b) bwd_rows slots 12-15 are scratch of the chain rule
 * (band views keep the compact live-row list there); (c) point_list tails of streamed lists (> 4096 keys) are unspecified
 * until lograst_finish_lists, which now checks that `keys` is the buffer the forward filled and synchronises the stream;
 * (d) lograst_view gained hit_masks / hit_mask_words / hit_mask_form: an optional buffer in which the forward leaves its
 * per-chunk hit masks for the reverse walk (below); new entry points: lograst_hit_mask_bytes, lograst_forward_form,
 * lograst_pack_rows_clear, lograst_unpack_rows(atomic = 2), lograst_activate_backward_adam.  Added later in round 6 without a
 * version change (new entry points only): lograst_pack_rows_hinted, lograst_add_visible, lograst_add_visible_n.
 * 2: lograst_view gained cov3d_precomp / dl_dcov3d; 3: the backward accumulates into 64-byte rows (bwd_rows); lograst_view gained walk_form.  Added since without a version change (new entry points only): lograst_sparse_segment_floats / lograst_pack_rows / lograst_unpack_rows / lograst_ordered_lengths / lograst_finish_lists.
 * lograst_recomposite / lograst_record_bytes and the profiling slot "recolor" (LOGRAST_NUM_KERNELS 22 -> 23, appended) are
 * additions within version 4, as is lograst_backward_form: no existing entry point, layout or default changed.  So are the
 * aux-channel entry points lograst_forward_aux / lograst_forward_render_aux / lograst_forward_speculative_aux /
 * lograst_backward_aux (new entry points only; lograst_view is untouched; bwd_rows slots 9-11 and, in that call, 12-14 are theirs). */
#define LOGRAST_TILE 16        /* pixels per tile side (tile rects are part of the integer contract) */
#define LOGRAST_REC_FLOATS 16  /* floats per projected-Gaussian record (64 B): see log_amd/csrc/project.hip */
/* The reverse walk's accumulators: ONE 64-byte row per Gaussian -- slots 0-1 dL/d(ndc mean x, y), 2-4 dL/d(conic A, B, C),
 * 5 dL/dopacity, 6-8 dL/dcolour r g b, 9-11 unused (lograst_backward_aux: dL/daux colour r g b; it also keeps the aux
 * image's dL/d(conic A, B, C) in 12-14), 12-15 scratch of the chain rule (band views keep the compact list of
 * the live rows there: row 0 its length, rows 1.. four indices each; whatever the caller finds in bwd_rows after
 * lograst_backward is unspecified).  A memory-side atomic costs one operation per 64-byte line whatever the number of lanes
 * in it (tools/micro/atomic_lines.hip), so a (wave, Gaussian) visit commits all nine sums as one. */
#define LOGRAST_BWD_ROW_FLOATS 16

/* 2-D low-pass flavours */
#define LOGRAST_FILTER_NONE 0   /* use_filter=False of the fork (LoG/render/renderer.py:151-152) */
#define LOGRAST_FORM_AUTO 0
#define LOGRAST_FORM_ROWS 1
#define LOGRAST_FORM_QUADRANT 2
#define LOGRAST_FILTER_DILATE 1 /* upstream package: cov.xx += 0.3 (LoG/model/geometry.py:87-88) */
#define LOGRAST_FILTER_CLAMP 2  /* `wodilate` fork: cov.xx = max(cov.xx, 0.3) (LoG/cuda/compute_radius_kernel.cu:100-104) */

/* Caller-owned status block of the forward (device words; see lograst_forward_render) */
#define LOGRAST_STATUS_WORDS 8
#define LOGRAST_STATUS_OVERFLOW 0        /* sticky: bit 0 set by every forward that overflowed */
#define LOGRAST_STATUS_LAST_INSTANCES 1  /* the most recent forward: tile instances, ... */
#define LOGRAST_STATUS_LAST_OVERFLOW 2   /* ... whether it overflowed, ... */
#define LOGRAST_STATUS_LAST_MAX_LEN 3    /* ... its longest tile list, ... */
#define LOGRAST_STATUS_LAST_RECT 4       /* ... and its rect-rule instance count */
#define LOGRAST_STATUS_MAX_INSTANCES 5   /* running maxima over all forwards since the caller cleared the block */
#define LOGRAST_STATUS_MAX_MAX_LEN 6
#define LOGRAST_STATUS_FORWARDS 7        /* forwards recorded since then */
/* A lograst_recomposite records itself as a forward: it repeats the instance count, longest list, rect count and overflow
 * verdict of the forward whose lists it walks in the LAST_* words, takes part in the running maxima and in FORWARDS, and
 * never raises the sticky bit of LOGRAST_STATUS_OVERFLOW (it fills nothing, so it cannot overflow anything; a forward
 * that did overflow raised the bit itself, and a recomposite over its lists renders nothing, like that forward). */

/* error codes */
#define LOGRAST_OK 0
#define LOGRAST_ERR_ARG -1
#define LOGRAST_ERR_HIP -2

/* Per-call view description.  Stands for GaussianRasterizationSettings
 * (/root/reference/LoG/render/renderer.py:63-76): image_height/width, tanfovx/y, bg, scale_modifier,
 * viewmatrix, projmatrix.  sh_degree/campos/prefiltered/debug have no effect on this path (LoG always
 * passes colors_precomp, renderer.py:72-75,144-145). */
typedef struct lograst_view {
  int32_t width, height;
  float tanfovx, tanfovy;
  float scale_modifier;
  int32_t filter_mode;     /* LOGRAST_FILTER_* */
  int32_t ndc_cull;        /* 1: also cull |ndc.x|,|ndc.y| > 1.3 (compute_radius_kernel.cu:131-134) */
  int32_t extras;          /* 1: produce the fork's point_id_pixel / point_weight_pixel / point_weight */
  const float* viewmatrix; /* device, 16 floats */
  const float* projmatrix; /* device, 16 floats */
  const float* bg;         /* device, 3 floats */
  /* Image split across GPUs ("per-GPU tile ownership"; new design, the reference is single-GPU): only
   * the tile rows [tile_row_begin, tile_row_end) are rendered -- every Gaussian's rect is clipped to them, so lists,
   * image rows, gradients and point_weight cover this band only, radii is 0 for Gaussians that do not reach it, and
   * pixels outside the band come out as background.  Both 0 = the whole image. */
  int32_t tile_row_begin, tile_row_end;
  /* The rasterizer's `cov3D_precomp` argument (the third-party forward's alternative to scales + rotations; LoG itself
   * never passes it, /root/reference/LoG/render/renderer.py:134,149): device, n x 6 floats, the upper triangle
   * (xx, xy, xz, yy, yz, zz) of every Gaussian's world-space covariance, or NULL.  When set, `scales` / `rotations` are
   * not read (they may be NULL) and scale_modifier has no effect (it scales the `scales` only); the backward entry points
   * then write dL/dcov3D (n x 6, off-diagonal entries carry both symmetric positions: 2 x the matrix partial) to
   * `dl_dcov3d` and leave dl_dscales / dl_drotations (may be NULL) alone. */
  const float* cov3d_precomp;
  float* dl_dcov3d;
  /* Which form of the compositing kernels (speed only, never a result; knobs LOGRAST_FWD_ROWS / LOGRAST_BWD_ROWS = 2
   * follow it, 0 / 1 override it): LOGRAST_FORM_AUTO = the library decides from n alone; LOGRAST_FORM_ROWS = the wave's
   * four 16-lane rows walk their own 4x4 pixel blocks (views of tiny splats: few tile instances per Gaussian);
   * LOGRAST_FORM_QUADRANT = the whole wave walks its 8x8 quadrant.  The caller knows the view's instances per Gaussian
   * from earlier forwards (forward) or from this view's forward (backward). */
  int32_t walk_form;
  /* Optional (version 4; NULL = off): a buffer in which the forward's compositing kernels leave, per wave and 64-entry chunk
   * of a tile list they walked, which entries contributed -- row-split form: per 4x4 block, the entries some pixel of the
   * block accumulated (LOGRAST_HIT_MASKS=2: the ballot of the support tests, a superset); quadrant form: the ballot of
   * the support tests -- and from which the reverse walk of lograst_backward takes its visits instead of running the tests
   * (and gathering every record of a chunk) again.  A visit the masks leave out adds exactly zero to every sum: same
   * gradients up to the order of the float atomics.  Device, 32-byte aligned, hit_mask_words 64-bit words >= lograst_hit_mask_bytes(capacity, width, height) / 8,
   * uninitialised; the backward must be given the very buffer (contents untouched) of the forward whose tile_state it is
   * handed.  Speed only: 30 M Gaussians, reverse walk 640 -> see DESIGN.md section 4.
   * What lograst_backward does with a buffer it cannot use (the instance count lives on the device, so this is checked
   * there, by every workgroup of the reverse walk, without a host synchronisation): if hit_mask_words holds fewer than
   * 16 * ((instances >> 6) + tiles) words -- the slots this view's lists index -- or if hit_mask_form is not the form the
   * forward recorded in tile_state when it wrote the masks, the walk reads NO word of the buffer and visits every entry of
   * every chunk instead.  That is a superset of any mask, so the gradients are those of a backward without hit_masks
   * (slower; no error is returned).  Contents changed after the forward are not detectable and give the sums of the
   * visits they name. */
  uint64_t* hit_masks;
  uint64_t hit_mask_words;
  /* lograst_backward only: what lograst_forward_form() returned for the forward's view (1 row-split, 2 quadrant; 0 = do not
   * use the masks).  The reverse walk takes the masks only when it runs in that same form (walk_form / LOGRAST_BWD_ROWS)
   * and the forward wrote them in it (above). */
  int32_t hit_mask_form;
} lograst_view;

int lograst_version(void);
const char* lograst_last_error(void);

/* ---- sizing helpers --------------------------------------------------------------------------- */
/* bytes of the per-tile state block for a WxH image and n Gaussians (header, counters, offsets, cursors, dispatch
 * order, and the per-batch slot reservations of the projection stage, which grow with n) */
size_t lograst_tile_state_bytes(int32_t width, int32_t height, int32_t n);
/* bytes of the projected-record array for N Gaussians (64-byte records followed by 16-byte fill records and a 4-byte
 * index each, then -- round 5 -- the rank rows of the rects of 5..16 tiles: 32 bytes per such rect, room for one in four
 * Gaussians of every projection batch: 8 bytes per Gaussian + 256 KB).  Records of Gaussians with radii == 0 are
 * undefined: a view that owns a band of tile rows does not write them (a Gaussian without a rect then costs the 40 bytes
 * its rect is computed from and its radii word). */
size_t lograst_geom_bytes(int32_t n);
/* bytes of the N 64-byte records alone -- the only part of `geom` that the compositing kernels and lograst_backward read
 * (fill records, indices and rank rows are the binning stage's): the size of lograst_recomposite's `records` */
size_t lograst_record_bytes(int32_t n);
/* bytes of the (depth,id) key buffer (keys + an equally large scratch half used by the long-list sort) / of the
 * sorted id list, for `capacity` tile instances */
size_t lograst_keys_bytes(uint32_t capacity);
/* bytes of lograst_view.hit_masks for `capacity` tile instances on a width x height image: 128 per (tile, 64-entry chunk)
 * slot, capacity / 64 + tiles + 1 slots (only the chunks a view walks are ever written or read) */
size_t lograst_hit_mask_bytes(uint32_t capacity, int32_t width, int32_t height);
/* which form the forward's compositing kernels take for this view (its walk_form + the LOGRAST_FWD_ROWS knob): 1 = row-split,
 * 2 = quadrant, negative = error.  Pass it back as hit_mask_form of the backward's view. */
int lograst_forward_form(const lograst_view* view);
/* which form the reverse walk of lograst_backward takes for this view of n Gaussians (its walk_form, the LOGRAST_BWD_ROWS
 * knob, and n against LOGRAST_HELPER_MIN_N): 1 = row-split, 2 = quadrant, negative = error. */
int lograst_backward_form(const lograst_view* view, int32_t n);
size_t lograst_list_bytes(uint32_t capacity);

/* ---- A0: LoG/cuda compute_radius --------------------------------------------------------------
 * Replaces compute_radius_module.compute_radius (/root/reference/LoG/cuda/compute_radius_kernel.cu:158-187;
 * caller LoG/model/level_of_gaussian.py:81-84): projected 3-sigma radius in pixels (float, no ceil),
 * 0 where |ndc| > 1.3 or det == 0. */
int lograst_compute_radius(int32_t p, const float* means3d, const float* scales, const float* rotations,
                           const float* projmatrix, const float* viewmatrix, float focal_x, float focal_y,
                           float tanfovx, float tanfovy, float* radii_out, void* stream);

/* ---- forward, stage 1: projection + tile counting + scan (A1, A2) -----------------------------
 * Stands for the first half of GaussianRasterizer.forward (called at LoG/render/renderer.py:153,190-198;
 * LoG/model/level_of_gaussian.py:211-219).  Writes radii[n] (API output), geom (n records), and
 * tile_state (per-tile counts/offsets).  The total number of tile instances is left in
 * tile_state and, if num_instances_host != NULL (pinned or pageable host memory), also copied there
 * after a stream synchronise so the caller can size the key/list buffers exactly; max_tile_len_host (optional)
 * receives the longest tile list, which stage 2 uses to launch only the sort levels that are needed.
 * geom must hold lograst_geom_bytes(n) and tile_state lograst_tile_state_bytes(width, height, n) bytes for THIS n
 * (both grow with n: per-Gaussian fill records, per-batch slot reservations). */
int lograst_forward_project(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                            const float* rotations, const float* opacities, const float* colors,
                            int32_t* radii, void* geom, void* tile_state, uint32_t* num_instances_host,
                            uint32_t* max_tile_len_host, void* stream);

/* ---- forward, stage 2: per-tile bucketing + per-tile depth sort + compositing (A3, A4, A5, A7, A8)
 * keys: scratch of lograst_keys_bytes(capacity) (dead after the call -- unless lograst_finish_lists is to complete
 * lazily ordered lists, see there); point_list: lograst_list_bytes(capacity), kept for backward: the ids of every tile
 * list in (depth, id) order as far as the view's walk needed them (all of a list of up to 4096 keys; at least the first
 * window of a longer one: lograst_ordered_lengths).  `capacity` = number of tile instances the two buffers can hold.  With the
 * exact count from stage 1 it always suffices.  With a guess (sync-free operation) the kernels never write past
 * it: if the real count is larger NOTHING is rendered, the overflow flag in tile_state is raised, and the
 * caller finds out from lograst_read_state() (the call itself cannot know without a host sync).
 * max_tile_len: host-side upper bound on the longest tile list (from stage 1, or a hint; 0 = unknown, treated
 * as `capacity`): lists longer than 8192 keys take a multi-pass sort whose number of launches depends on it.  An
 * under-estimate leaves such lists partially sorted, so pass 0 when in doubt.
 * Outputs: image[3,H,W], final_T[H,W], n_contrib[H,W] (both kept for backward), and when
 * view->extras: point_id_pixel[H,W] (i32, -1 = none), point_weight_pixel[H,W], point_weight[n].
 * bwd_scratch (optional, NULL/0 = none; bwd_scratch_floats must be 0 or LOGRAST_BWD_ROW_FLOATS): the n x 16 fp32
 * accumulator rows of lograst_backward (its `bwd_rows`), zero-filled here (inside a kernel this call launches anyway) for
 * a caller that will differentiate this view: pass the block to lograst_backward with LOGRAST_BWD_SCRATCH_ZEROED -- no
 * separate memset.  With view->extras on large inputs (n >= 4,000,000, env LOGRAST_HELPER_MIN_N) only the rows of
 * Gaussians that contributed to a pixel are cleared (point_weight > 0; the compositing kernel clears a row when it meets
 * the Gaussian; below that size the whole block is cleared): always pass point_weight and
 * LOGRAST_BWD_CONIC_TOUCHED_ONLY to lograst_backward after a forward with view->extras (correct at every size;
 * lograst_backward rejects LOGRAST_BWD_SCRATCH_ZEROED without point_weight on large inputs).
 * max_tile_len is also CHECKED on the device: when the real longest list exceeds a non-zero max_tile_len (or the
 * instance count exceeds capacity) nothing is sorted or composited and the overflow flag of tile_state is raised; the
 * outputs of such a call are undefined.  status (optional): LOGRAST_STATUS_WORDS device words owned by the caller
 * (zeroed once), into which every forward records itself -- see LOGRAST_STATUS_* -- so that a caller running many
 * sync-free forwards, on any number of streams, checks all of them with one read-back.
 * bwd_scratch must be 64-byte aligned. */
int lograst_forward_render(const lograst_view* view, int32_t n, const void* geom, void* tile_state,
                           uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                           float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                           float* point_weight_pixel, float* point_weight, float* bwd_scratch,
                           int32_t bwd_scratch_floats, uint32_t* status, void* stream);

/* ---- forward in ONE call (sync-free operation) ---------------------------------------------------------------
 * lograst_forward_project + lograst_forward_render back to back for a caller that already knows a capacity (and a
 * max_tile_len, or 0): one boundary crossing and no host decision between the stages -- what GaussianRasterizer.forward
 * (LoG/render/renderer.py:153) costs the host is then one call.  Arguments as in the two stage calls. */
int lograst_forward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                    const float* rotations, const float* opacities, const float* colors, int32_t* radii, void* geom,
                    void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                    float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                    float* point_weight_pixel, float* point_weight, float* bwd_scratch, int32_t bwd_scratch_floats,
                    uint32_t* status, void* stream);

/* ---- the same Gaussians, other colours: a second compositing pass over a forward's tile lists ---------------------------
 * LoG's depth pass (render_depth: True, LoG/render/renderer.py:186-201) calls the rasterizer a second time with the same
 * means3D / opacities / scales / rotations and colors_precomp = [view depth, world z, 1].  Nothing a forward bins, counts,
 * scans, fills or sorts depends on the colours, so this entry point produces the stage-2 outputs of such a second forward
 * from the FIRST forward's radii / geom / tile_state / point_list (all four only read -- the compositing kernels store
 * into tile_state nothing but the open[] bits and header words it already holds --, so that forward's lograst_backward
 * may still run afterwards): one streaming kernel copies the records into `records` (lograst_record_bytes(n), 16-byte
 * aligned, not geom itself) with the colour fields replaced from colors[n,3], writes radii_out[n] (= radii: an array of
 * the second call's own), clears point_weight[n] and bwd_scratch as lograst_forward_render does; then the compositing
 * launch(es) of a stage 2 run over `records`.  No fill, no sort, no host read-back: capturable like lograst_forward.
 * capacity / max_tile_len: the values the first forward's stage 2 ran with (they decide, as there, whether long lists
 * are walked lazily: the second walk parks and resumes exactly where the first did, over tails that the first forward
 * ordered).  view: the first forward's (same matrices, filter, walk_form, whole image: a band is an error), with a
 * hit_masks buffer OF ITS OWN when the second call is to be differentiated with masks.  Outputs as lograst_forward_render;
 * lograst_backward then takes (radii_out, records, tile_state, point_list, final_t, n_contrib, bwd_scratch,
 * point_weight) of this call.  status: see LOGRAST_STATUS_*.  Results are bit for bit those of a full forward with
 * `colors`. */
int lograst_recomposite(const lograst_view* view, int32_t n, const int32_t* radii, const void* geom,
                        const void* tile_state, const uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                        const float* colors, void* records, int32_t* radii_out, float* image, float* final_t,
                        int32_t* n_contrib, int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight,
                        float* bwd_scratch, int32_t bwd_scratch_floats, uint32_t* status, void* stream);

/* The forward in one call for a caller that has only a GUESS of the capacity (and of max_tile_len): what the drop-in
 * package's default mode runs (log_amd/rasterizer.py).  Stage 1, then stage 2 with the guessed buffers are enqueued back
 * to back -- the stream never waits for the host --, while the stage-1 header {instance count, longest list} is copied
 * to the host on an internal side stream that waits for stage 1 only; the call returns once that copy has landed
 * (stage 2 is then still running or queued).  If *num_instances_host <= capacity and (max_tile_len == 0 or
 * *max_tile_len_host <= max_tile_len) the speculative stage 2 is the forward.  Otherwise its kernels returned without
 * rendering (as in lograst_forward_render with too small a capacity) and the caller repeats stage 2 alone with exact
 * buffers: lograst_forward_render(view, n, geom, tile_state, <keys / point_list for *num_instances_host>, ...).  An
 * attempt that overflows does not touch `status` (the repeat records the forward).  Synchronises the side stream, not
 * `stream`; not capturable into a HIP graph (use lograst_forward with a known capacity there).  Stands for the
 * num_rendered read-back of the third-party forward (called at LoG/render/renderer.py:153) without its pipeline bubble. */
int lograst_forward_speculative(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                const float* rotations, const float* opacities, const float* colors, int32_t* radii,
                                void* geom, void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity,
                                uint32_t max_tile_len, float* image, float* final_t, int32_t* n_contrib,
                                int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight,
                                float* bwd_scratch, int32_t bwd_scratch_floats, uint32_t* status,
                                uint32_t* num_instances_host, uint32_t* max_tile_len_host, void* stream);

/* Aux channels: a second colour triple per Gaussian, aux_colors [n, 3] fp32, composited into aux_image [3, H, W] by the SAME
 * walk that produces `image` -- one list fetch, one record gather, one support decision, one alpha evaluation, one T and
 * stop test per visit, three more fused multiply-adds per contributing pixel.  The three sums are accumulated with the same
 * weights, in the same list order, with the same fma as the RGB sums, and the image is written as fma(T, bg[c], sum) with
 * the view's own bg: aux_image has the bits of `image` from a second forward whose colors are aux_colors (LoG's depth pass:
 * [view z, world z, 1], LoG/render/renderer.py:186-201).  Every other output (radii, final_t, n_contrib, the fork's maps,
 * point_weight, hit masks, bwd_scratch) is what the entry point without _aux leaves.  The three calls below are
 * lograst_forward / lograst_forward_render / lograst_forward_speculative with (aux_colors, aux_image) behind `status`.
 * Quadrant form only: the compositing kernel is the quadrant one whatever view->walk_form or LOGRAST_FWD_ROWS say, and the
 * hit masks it leaves are quadrant masks (pass hit_mask_form = LOGRAST_FORM_QUADRANT to the backward).  LOGRAST_ERR_ARG
 * before any launch: aux_colors or aux_image NULL with n > 0; a band view (tile_row_begin / tile_row_end); cov3d_precomp. */
int lograst_forward_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                        const float* rotations, const float* opacities, const float* colors, int32_t* radii, void* geom,
                        void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                        float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                        float* point_weight_pixel, float* point_weight, float* bwd_scratch, int32_t bwd_scratch_floats,
                        uint32_t* status, const float* aux_colors, float* aux_image, void* stream);
int lograst_forward_render_aux(const lograst_view* view, int32_t n, const void* geom, void* tile_state,
                               uint64_t* keys, uint32_t* point_list, uint32_t capacity, uint32_t max_tile_len,
                               float* image, float* final_t, int32_t* n_contrib, int32_t* point_id_pixel,
                               float* point_weight_pixel, float* point_weight, float* bwd_scratch,
                               int32_t bwd_scratch_floats, uint32_t* status, const float* aux_colors, float* aux_image,
                               void* stream);
int lograst_forward_speculative_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                    const float* rotations, const float* opacities, const float* colors, int32_t* radii,
                                    void* geom, void* tile_state, uint64_t* keys, uint32_t* point_list, uint32_t capacity,
                                    uint32_t max_tile_len, float* image, float* final_t, int32_t* n_contrib,
                                    int32_t* point_id_pixel, float* point_weight_pixel, float* point_weight,
                                    float* bwd_scratch, int32_t bwd_scratch_floats, uint32_t* status, const float* aux_colors,
                                    float* aux_image, uint32_t* num_instances_host, uint32_t* max_tile_len_host, void* stream);

/* Image split into bands of tile rows (new design, SURVEY 8e / BASELINE configs[4]; view->tile_row_begin/end): the
 * tile-row range every Gaussian's rect covers on the WHOLE image, rows_out[i] = y0 | y1 << 16 (rows [y0, y1); 0 = the
 * projection drops this Gaussian), computed by the projection's own code: the Gaussians lograst_forward keeps for a band
 * [b, e) are exactly those with y0 < e and y1 > b.  A rank that owns a band renders from that subset only (same relative
 * order => same tile lists, bit-identical band).  view->tile_row_begin/end are ignored here. */
int lograst_tile_rows(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                      const float* rotations, uint32_t* rows_out, void* stream);

/* Measurement helper (bench.py's HBM denominator, SURVEY 8d "measured device-copy bandwidth"): streams `bytes` from
 * src to dst with 16-byte accesses.  `blocks` & 0xfffff = workgroups of 256 of the grid-stride forms (0: 4096);
 * `blocks` >> 20 = form: 0 grid-stride, four non-temporal loads in flight per lane, non-temporal stores; 1 one access
 * per lane, no loop, plain loads / stores; 2 as 0 with eight loads in flight; 3 as 0 with plain loads; 4 as 1,
 * non-temporal.  Pointers and size must be multiples of 16 bytes.  Not on the rasterizer's path. */
int lograst_stream_copy(void* dst, const void* src, size_t bytes, int32_t blocks, void* stream);

/* ---- row-sparse gradient exchange: pack / unpack (log_amd/dist.py; the reference has no multi-GPU code: new surface) ---
 * rows: float32 [groups][rows_per_group][16] -- a row-major running-sum bucket (LOGRAST_GRAD_ROW_FLOATS = 16), 64-byte
 * aligned.  lograst_pack_rows writes one SEGMENT per group, back to back, each lograst_sparse_segment_floats(kmax) floats:
 * header [16] (word 0: how many rows with a non-zero entry the group holds), values [kmax][16] (those rows, in no
 * particular order), index [roundup(kmax, 16)] (int32: the row's index inside its group).  Rows beyond kmax are dropped
 * and *overflow (a device word, OR-ed; may be NULL) is raised.  Value rows and index words j >= min(count, kmax) of a
 * segment are unspecified: nothing reads them.  Equal-sized segments: an all-to-all / all-gather with
 * equal splits moves them.  lograst_unpack_rows: for every segment s and every row j < min(count_s, kmax):
 *   atomic != 0:  dest[index][0..15] += values            (all segments into the same rows_per_group rows.  Despite the
 *                 argument's name no float atomics are involved since round 5: the segments are added one after the
 *                 other in segment order -- rows inside one segment are unique --, so a row's sum is
 *                 ((s0 + s1) + s2) + ... on every run, whatever order the segments arrived in)
 *   atomic == 0:  dest[s * dest_group_rows + index][..] = values   (segment s owns its own range of rows: plain stores;
 *                 dest_group_rows >= rows_per_group)
 *   atomic == 2:  dest[s * dest_group_rows + index][..] = 0        (version 4: clears exactly the rows an earlier
 *                 atomic == 0 call with the same segments wrote -- cheaper than zero-filling a mostly empty result)
 * dest and packed must be 16-byte aligned. */
size_t lograst_sparse_segment_floats(int32_t kmax);
int lograst_pack_rows(const float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                      uint32_t* overflow, void* stream);
/* lograst_pack_rows that also ZEROES every row it packed in `rows` ("pack and clear", version 4): the bucket of a group of
 * views is all zero again once its rows are on their way, so a step that streams its exchange group by group
 * (log_amd.dist.StepExchange, parts > 1, sparse) never zero-fills its buckets.  Rows dropped by an exceeded kmax stay. */
int lograst_pack_rows_clear(float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                            uint32_t* overflow, void* stream);
/* The same with a HINT (added late in round 6, new entry point only): `hint` holds one 32-bit word per row of the whole array
 * (row g * rows_per_group + r; rows from hint_rows on have none).  A row whose word is zero is, by the caller's contract, all
 * zero: it is neither read nor packed (nor cleared); a row whose word is non-zero is packed whatever it holds (an all-zero
 * row then travels as zeros).  The word is compared as bits: a view's point_weight [n] (float, zero
 * exactly for the Gaussians that contributed to no pixel -- lograst_backward leaves their gradient rows untouched) is such a
 * hint for a bucket that holds that ONE view's gradient rows: the scan then reads 4 bytes per row instead of 64.  clear != 0:
 * as lograst_pack_rows_clear. */
int lograst_pack_rows_hinted(float* rows, int32_t groups, int64_t rows_per_group, int32_t kmax, float* packed,
                             uint32_t* overflow, int32_t clear, const uint32_t* hint, int64_t hint_rows, void* stream);
int lograst_unpack_rows(float* dest, const float* packed, int32_t segments, int32_t kmax, int64_t rows_per_group,
                        int64_t dest_group_rows, int32_t atomic, void* stream);
/* seen[i] += 1 where radii[i] > 0, i < n (the per-step "how many views saw this row" counts of log_amd.dist: what the
 * reference's step calls flag_vis, /root/reference/LoG/model/counter.py:48,50, summed over a rank's views). */
int lograst_add_visible(float* seen, const int32_t* radii, int64_t n, void* stream);
/* The same for k <= 16 views in one pass: `radii` is a HOST array of k device pointers ([n] int32 each); seen[i] += the number
 * of them with radii[j][i] > 0. */
int lograst_add_visible_n(float* seen, const int32_t* const* radii, int32_t k, int64_t n, void* stream);

/* ---- performance knobs -------------------------------------------------------------------------------------------
 * Launch-shape parameters that change no result (thresholds, grid caps, dispatch orders; the list is enumerated by
 * lograst_knob_count / lograst_knob_info).  Each is the environment variable of the same name unless overridden here;
 * overrides take effect from the next launch.  Sizing helpers (lograst_tile_state_bytes) and the forward of one view must
 * see the same values: change knobs between views, not between a sizing call and its forward.  log_amd.tune() calibrates
 * them per device.  All return 0 or LOGRAST_ERR_ARG (unknown name / value outside [lo, hi]). */
int lograst_knob_count(void);
int lograst_knob_info(int32_t index, const char** name, int32_t* dflt, int32_t* lo, int32_t* hi, const char** what);
int lograst_set_knob(const char* name, int32_t value);
int lograst_get_knob(const char* name, int32_t* value);
int lograst_reset_knobs(void);

/* Copies {num_instances, overflow_flag, longest tile list, rect instances} of a tile_state to host (synchronises
 * the stream; any pointer may be NULL).  rect_instances = what the plain rect rule of the reference would have
 * binned (num_rendered of the third-party package); num_instances <= rect_instances when the support cull is on. */
int lograst_read_state(const void* tile_state, uint32_t* num_instances_host, uint32_t* overflow_host,
                       uint32_t* max_tile_len_host, uint32_t* rect_instances_host, void* stream);

/* Support cull in the binning stage (default on; also LOGRAST_TILE_CULL=0): a tile of a Gaussian's rect becomes
 * a list entry only if the Gaussian can reach alpha >= 1/255 somewhere inside it.  Result-preserving (dropped
 * entries fail the alpha floor at every pixel of the tile); with it off the tile lists are exactly the
 * reference's rect lists.  Process-wide; returns the previous setting. */
int lograst_set_tile_cull(int enabled);

/* ---- backward (A6, A6b) ------------------------------------------------------------------------
 * Stands for _RasterizeGaussians.backward of the third-party package, triggered by loss.backward()
 * (LoG/utils/trainer.py:158).  dL_dimage[3,H,W] in; all gradient outputs are overwritten:
 *   dL_dmeans2d[n,3]  (x,y = d/d ndc, z = 0; consumed at LoG/model/counter.py:40,46)
 *   dL_dmeans3d[n,3], dL_dscales[n,3], dL_drotations[n,4], dL_dopacities[n], dL_dcolors[n,3]
 * bwd_rows[n, LOGRAST_BWD_ROW_FLOATS] is scratch: the reverse walk's accumulator rows (64-byte aligned; the forward's
 * bwd_scratch, or any zeroed block); the chain-rule kernel reads each live Gaussian's row and writes the separate
 * outputs (dL_dmeans2d for every row; dL_dopacities / dL_dcolors written, or added to when accumulating).  rotations /
 * dl_drotations must be 16-byte aligned (one 16-byte access per Gaussian).  flags:
 *   LOGRAST_BWD_SCRATCH_ZEROED  bwd_rows is already zeroed (the forward's bwd_scratch; or the caller's memset);
 *   LOGRAST_BWD_ACCUMULATE      multi-view accumulation (new, not in the reference): dl_dopacities, dl_dcolors,
 *                               dl_dmeans3d, dl_dscales, dl_drotations are running sums that this call ADDS to
 *                               (the reverse walk's atomics and the chain-rule kernel write straight into the
 *                               caller's per-step gradient bucket; no separate accumulate pass).
 *   LOGRAST_BWD_CONIC_TOUCHED_ONLY  bwd_rows is zeroed only in the rows of Gaussians with point_weight > 0 (what a
 *                               forward with extras and a bwd_scratch leaves on large inputs: see lograst_forward_render);
 *                               needs point_weight.  (Documentation of the caller's state: the chain rule skips the
 *                               rows with point_weight == 0 whenever point_weight is given, with or without this flag.)
 * point_weight (optional, NULL = none): the forward's per-Gaussian maximum blend weight.  A Gaussian with weight 0
 * contributed to no pixel, so its dL/dmean2D and dL/dconic are exactly zero: the chain rule skips it (its gradients
 * are written as 0, or left alone when accumulating) without reading its inputs -- in an opaque scene that is most of
 * the Gaussians.  It must be the UNMODIFIED point_weight output of the forward whose geom / tile_state / point_list are
 * passed here: the forward clears it for every row and only composited Gaussians (radii > 0) ever raise it, so the kernel
 * takes point_weight > 0 alone as the live flag and does not read radii for that decision.
 * Alignment: bwd_rows 64 bytes; rotations / dl_drotations 16 bytes; every other array 4 bytes (the kernels' full-width
 * clears of dl_dmeans2d / dl_dopacities / dl_dcolors / dl_dmeans3d / dl_dscales / dl_dcov3d start with a scalar head). */
#define LOGRAST_BWD_SCRATCH_ZEROED 1
#define LOGRAST_BWD_ACCUMULATE 2
#define LOGRAST_BWD_CONIC_TOUCHED_ONLY 4
/* multi-view accumulation into ONE 64-byte row per Gaussian (new): dl_dmeans3d points to the caller's running sums
 * [n][LOGRAST_GRAD_ROW_FLOATS] (64-byte aligned; slots 0-2 dL/dmeans3D, 3-5 dL/dscales, 6-9 dL/drotations, 10 dL/dopacity,
 * 11-13 dL/dcolour, 14-15 never touched) and every gradient of this view is ADDED there; dl_dscales, dl_drotations,
 * dl_dopacities, dl_dcolors are not used (NULL allowed).  A Gaussian that composited somewhere then costs the chain rule
 * one read-modify-write of one line instead of five pieces in five arrays (log_amd.dist.GradientBucket(row_major=True)).
 * Not with cov3d_precomp. */
#define LOGRAST_BWD_ACCUMULATE_ROWS 8
#define LOGRAST_GRAD_ROW_FLOATS 16

int lograst_backward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                     const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                     const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                     const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                     float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                     const float* point_weight, int32_t flags, void* stream);

/* The backward of a lograst_forward*_aux call: ONE reverse walk and ONE chain-rule launch for both images.  dl_dimage and
 * dl_daux_image are the gradients of `image` and `aux_image` ([3, H, W] each); either may be NULL = zeros, not both.
 * dL/dalpha is evaluated per image; fifteen per-Gaussian sums leave in four atomic instructions on the Gaussian's one 64-byte
 * row of bwd_rows (bwd_row_floats must be LOGRAST_BWD_ROW_FLOATS: slots 9-11 take dL/daux colour, slots 12-14 the aux
 * image's dL/dconic, kept apart from the image's in 2-4), and the chain rule writes dl_daux_colors [n, 3] next to dl_dcolors
 * (zeros for Gaussians that composited nowhere).  dl_dmeans2d and the geometry gradients are the sums over both images; the
 * conic part of the chain rule -- ill-conditioned in fp32 for needle-shaped Gaussians -- runs once per image inside the one
 * launch and the results are added, which is the arithmetic of two lograst_backward calls.  Fresh gradients only: flags may hold
 * LOGRAST_BWD_SCRATCH_ZEROED and LOGRAST_BWD_CONIC_TOUCHED_ONLY.  Quadrant form only (view->hit_masks are read when
 * hit_mask_form = LOGRAST_FORM_QUADRANT).  LOGRAST_ERR_ARG before any launch: a band view; cov3d_precomp; aux_colors or
 * dl_daux_colors NULL; both image gradients NULL; bwd_row_floats != 16; LOGRAST_BWD_ACCUMULATE / _ACCUMULATE_ROWS. */
int lograst_backward_aux(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                         const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                         const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                         const float* aux_colors, const float* dl_dimage, const float* dl_daux_image, float* dl_dmeans2d,
                         float* bwd_rows, int32_t bwd_row_floats, float* dl_dopacities, float* dl_dcolors,
                         float* dl_daux_colors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                         const float* point_weight, int32_t flags, void* stream);

/* Stage A6b alone: the per-Gaussian chain rule, given dL/d(ndc mean) [n,3] and dL/d(conic) [n,4] (as left
 * by the reverse walk).  Writes dl_dmeans3d/dl_dscales/dl_drotations.  lograst_backward = reverse walk +
 * this call; exposed so the two halves can be checked separately (the chain rule is ill-conditioned for
 * near-degenerate Gaussians, the walk is not). */
int lograst_project_backward(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                             const float* rotations, const int32_t* radii, const float* dl_dmeans2d,
                             const float* dl_dconic, float* dl_dmeans3d, float* dl_dscales,
                             float* dl_drotations, void* stream);

/* Camera gradients: lograst_backward / lograst_project_backward once more, with dL/dviewmatrix and dL/dprojmatrix as two
 * further outputs ([4, 4] fp32 each, row-major, the layout of view->viewmatrix / view->projmatrix; written whole, never
 * added to).  The chain-rule launch sums them over the Gaussians it differentiates, the terms evaluated in double (the fp32
 * chain is ill-conditioned on needle-shaped Gaussians, and these sums are much smaller than their terms):
 * with t = [p 1] V the view-space centre, T = J V[:3,:3]^T the EWA factor and hom = [p 1] P,
 *   dL/dV[j][k] = sum dL/dT-terms + p_j dL/dt_k,  dL/dV[3][k] = sum dL/dt_k   (k = 0..2; dL/dt behind the 1.3 tan(fov) clamps),
 *   dL/dP[j][c] = sum p_j dL/dhom_c,              dL/dP[3][c] = sum dL/dhom_c (c = 0, 1, 3).
 * Column 3 of dL/dviewmatrix and column 2 of dL/dprojmatrix are exactly 0: no output depends on them.  Each workgroup stores
 * its 24 partial sums to camera_scratch (lograst_camera_scratch_bytes(n) bytes of device memory, 8-byte aligned; its content
 * afterwards is unspecified) and a finishing kernel (two above 2 M Gaussians) adds them in workgroup order in double: no float atomics, and identical
 * inputs give identical bits.  Every other output is what the entry point without _camera writes (the per-Gaussian results
 * of lograst_project_backward_camera bit for bit).  n == 0, or no live Gaussian: zeros.  view->campos does not exist in
 * this ABI; a native-SH colour's dependence on the camera position is outside these gradients.
 * Fresh gradients only, scales / rotations form, whole images.  LOGRAST_ERR_ARG before any launch: LOGRAST_BWD_ACCUMULATE or
 * LOGRAST_BWD_ACCUMULATE_ROWS in flags; view->cov3d_precomp; a band view (tile_row_begin / tile_row_end); a NULL gradient
 * matrix; a scratch that is NULL or too small.  There is no camera form of lograst_backward_aux.  (Additions within
 * version 4: new entry points only, lograst_view untouched.) */
size_t lograst_camera_scratch_bytes(int32_t n);
int lograst_backward_camera(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                            const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                            const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                            const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                            float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                            const float* point_weight, int32_t flags, float* dl_dviewmatrix, float* dl_dprojmatrix,
                            void* camera_scratch, size_t camera_scratch_bytes, void* stream);
int lograst_project_backward_camera(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                                    const float* rotations, const int32_t* radii, const float* dl_dmeans2d,
                                    const float* dl_dconic, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                                    float* dl_dviewmatrix, float* dl_dprojmatrix, void* camera_scratch,
                                    size_t camera_scratch_bytes, void* stream);

/* Absolute screen-space gradients (the AbsGS densification statistic; gsplat: `absgrad`): lograst_backward once more, with
 * one further output dl_dmeans2d_abs [n, 3] (fp32, overwritten):
 *   dl_dmeans2d_abs[g, 0] = sum over pixels | dL/dG dG/ddx 0.5 W |,  [g, 1] = sum over pixels | dL/dG dG/ddy 0.5 H |,  [g, 2] = 0
 * -- the absolute values of the very fp32 per-pixel terms whose signed sums are dl_dmeans2d[g, 0..1], taken per pixel and
 * per component in front of any reduction; units and scaling are dl_dmeans2d's.  The signed terms are odd around the splat
 * centre and cancel for a large splat inside the image; these do not.  A Gaussian that contributed to no pixel gets exact
 * zeros.  The reverse walk sums them into slots 9 and 10 of the Gaussian's accumulator row (the row-split form: eleven lanes
 * of the one atomic instruction of a row visit; the quadrant form: two more lanes of its second atomic instruction), the
 * chain rule hands them out.  Every other output is what lograst_backward writes (sums up to the order of the float atomics).
 * The walk form follows lograst_backward_form as lograst_backward's does; view->hit_masks are read in either form.
 * Fresh gradients only, scales / rotations form, whole images: flags may hold LOGRAST_BWD_SCRATCH_ZEROED and
 * LOGRAST_BWD_CONIC_TOUCHED_ONLY.  LOGRAST_ERR_ARG before any launch: a band view (tile_row_begin / tile_row_end);
 * view->cov3d_precomp; LOGRAST_BWD_ACCUMULATE / LOGRAST_BWD_ACCUMULATE_ROWS; dl_dmeans2d_abs NULL.  There is no abs form of
 * lograst_backward_aux or lograst_backward_camera.  (An addition within version 4: a new entry point only.) */
int lograst_backward_abs(const lograst_view* view, int32_t n, const float* means3d, const float* scales,
                         const float* rotations, const int32_t* radii, const void* geom, const void* tile_state,
                         const uint32_t* point_list, const float* final_t, const int32_t* n_contrib,
                         const float* dl_dimage, float* dl_dmeans2d, float* bwd_rows, float* dl_dopacities,
                         float* dl_dcolors, float* dl_dmeans3d, float* dl_dscales, float* dl_drotations,
                         const float* point_weight, int32_t flags, float* dl_dmeans2d_abs, void* stream);

/* ---- "next" row N1: simple_knn._C.distCUDA2 ----------------------------------------------------------
 * Replaces distCUDA2 (third-party simple-knn, un-vendored; called at /root/reference/LoG/utils/file.py:88-91 and
 * LoG/model/base_gaussian.py:39-42): out[i] = mean squared distance from point i to its 3 nearest other
 * points (exact, fp32).  scratch: lograst_knn_scratch_bytes(p) bytes of device memory.  Exactly p floats of `out` are
 * written.  p < 4: a point has fewer than three other points and out[i] is unspecified (some non-NaN float; a caller that
 * may see such a cloud chooses its own scale). */
size_t lograst_knn_scratch_bytes(int32_t p);
int lograst_knn_mean_dist2(int32_t p, const float* points, float* out, void* scratch, size_t scratch_bytes,
                           void* stream);

/* ---- "next" row N2: the packages' native `shs=` input --------------------------------------------------
 * colours[n,3] = max(0, 0.5 + sum_{k < (deg+1)^2} basis_k(normalise(mean - campos)) * shs[n,k,:]), shs laid out
 * [n, max_coeffs, 3]; clamped[n*3] (u8) records which channels hit the clamp.  Backward: dl_dshs[n,max_coeffs,3]
 * is overwritten (accumulate = 0) or added to (accumulate != 0: running sums over views), the direction gradient
 * is ADDED to dl_dmeans3d.  (Third-party package's computeColorFromSH;
 * LoG passes colors_precomp instead, LoG/render/renderer.py:144-145.)
 * Alignment: every pointer needs the alignment of its element type only (4 bytes for the float arrays).  shs and dl_dshs
 * move as 16-byte accesses when 3 * max_coeffs % 4 == 0 and the pointer is 16-byte aligned, one float at a time
 * otherwise; both ways give the same bits. */
int lograst_sh_forward(int32_t n, int32_t degree, int32_t max_coeffs, const float* means3d, const float* campos,
                       const float* shs, float* colors, uint8_t* clamped, void* stream);
int lograst_sh_backward(int32_t n, int32_t degree, int32_t max_coeffs, const float* means3d, const float* campos,
                        const float* shs, const uint8_t* clamped, const float* dl_dcolors, float* dl_dshs,
                        float* dl_dmeans3d, int32_t accumulate, void* stream);

/* ---- debugging / test access to intermediates --------------------------------------------------
 * Pointers into a tile_state block (device): offsets has tiles+1 entries. */
const uint32_t* lograst_tile_offsets(const void* tile_state, int32_t width, int32_t height);
/* Lazily ordered tile lists (knob LOGRAST_LAZY_SORT, default on).  The third-party package sorts every (tile, depth) key
 * of a view (one global radix sort) before it composites; this library orders, of a list of more than 4096 keys, only
 * the first window (7680 positions, cut at a depth-bucket boundary) before the compositing pass, lets that pass mark the
 * tiles in which a pixel was still open at the end of the ordered part, and then orders the rest of exactly those lists
 * and composites their tiles again.  Images, fork maps, n_contrib, point_weight and every gradient are the same bit for
 * bit either way (tests/test_gpu_knobs.py); what differs is point_list behind the ordered part of a list nobody walked:
 * those entries are unspecified until lograst_finish_lists has run.
 *   lograst_ordered_lengths: lengths_out[t] (device, tiles entries) = leading positions of tile t's list that are in
 *     final order (the whole list for lists of up to 4096 keys, and for every list when the knob is 0);
 *   lograst_finish_lists: orders every list to its end (same tile_state / keys / point_list / capacity as the forward
 *     call, before any other forward reuses the keys buffer).  The lists are then what LOGRAST_LAZY_SORT=0 produces. */
int lograst_ordered_lengths(const void* tile_state, int32_t width, int32_t height, uint32_t* lengths_out, void* stream);
int lograst_finish_lists(void* tile_state, int32_t width, int32_t height, void* keys, uint32_t* point_list,
                         uint32_t capacity, void* stream);

/* ---- "next" row N3: level-of-detail selection ------------------------------------------------------------
 * Replaces TensorTree.traverse + TensorTree._query_tree_torch (/root/reference/LoG/model/tensor_tree.py:131-185;
 * caller LoG.prepare, LoG/model/level_of_gaussian.py:241) together with the Gaussian.compute_radius it calls per
 * level (level_of_gaussian.py:65-88: gather, exp / normalize activations, compute_radius_module.compute_radius).
 * Inputs are the tree buffers as TensorTree keeps them (node_index i32[num_points], -1 = leaf; tree
 * i32[num_nodes, max_child], -1 = removed child), the RAW model parameters (xyz[P,3], log-scales[P,3],
 * unnormalised quaternions[P,4]), the roots to start from (i64[num_roots]) and the camera of
 * lograst_compute_radius.  `levels` = number of levels to expand below the roots = min(tree.max_level, max_depth)
 * of the reference call (values beyond the tree's depth cost only empty launches).
 * out_index (i64, capacity out_capacity >= num_points is always enough: a point is selected at most once)
 * receives, in the reference's order, [roots kept | children kept at level 1 | ... | frontier left at the depth
 * limit], keep = (radius < min_resolution_pixel) | is_leaf.  The count stays on the device; read it with
 * lograst_lod_read (one stream synchronise -- the only one; the reference synchronises several times per level).
 * scratch: lograst_lod_scratch_bytes(num_roots, num_nodes, max_child) bytes. */
size_t lograst_lod_scratch_bytes(int32_t num_roots, int32_t num_nodes, int32_t max_child);
int lograst_lod_traverse(int32_t num_points, int32_t num_nodes, int32_t max_child, const int32_t* node_index,
                         const int32_t* tree, const float* xyz, const float* scaling, const float* rotation,
                         const int64_t* root_index, int32_t num_roots, const float* projmatrix,
                         const float* viewmatrix, float focal_x, float focal_y, float tanfovx, float tanfovy,
                         float min_resolution_pixel, int32_t levels, int64_t* out_index, uint32_t out_capacity,
                         void* scratch, size_t scratch_bytes, void* stream);
/* count_host / overflow_host / frontier_left_host: host words (the last two optional).  overflow != 0 means the
 * tree buffers were inconsistent (a point reachable twice) and out_index is incomplete.  frontier_left = how many of
 * the selected points are nodes that were still waiting to be expanded when `levels` ran out (0 whenever `levels`
 * reached the bottom of the tree): a caller that passes a cached tree depth as `levels` re-runs with the full value
 * if this is not 0. */
int lograst_lod_read(const void* scratch, uint32_t* count_host, uint32_t* overflow_host, uint32_t* frontier_left_host,
                     void* stream);

/* ---- view preparation: LoG.prepare, Gaussian.prepare and LoG.clamp_scale on the device ---------------------------
 * (/root/reference/LoG/model/level_of_gaussian.py:39-53, :90-98, :223-256, :367-398; Python side: log_amd/prepare.py).
 * No call allocates; all work on `stream`.
 *
 * lograst_frustum_select = Gaussian._visible_flag_by_camera + the boolean-mask indexing behind it.  Entry i < n is row
 * rows[i] (i32, as TensorTree keeps root_index) or row i when rows == NULL; xyz is [num_points, 3]; full_proj the 4x4
 * full_proj_transform, row-major, applied as [x, y, z, 1] @ M.  flag_out u8[n] = (0 < z' < 1) & (|x'|, |y'| < 1 +
 * padding), p' = h / (hw + 1e-7), strict comparisons in fp32 (a NaN or an infinity anywhere, or a row outside
 * [0, num_points), gives 0).  pos_out i64 (capacity n) receives the positions i of the kept entries in ascending order,
 * row_out (optional, same capacity) their rows.  With the raw scaling[P,3], rotation[P,4] and opacity[P] given (all
 * three, and the four outputs, or none), xyz_out[.,3], scaling_out[.,3] = exp, rotation_out[.,4] = normalised and
 * opacity_out[.] = sigmoid hold the kept entries' parameters in the same order (capacity n rows each), bit for bit what
 * lograst_gather_activate writes for those rows.  The count stays on the device: lograst_frustum_read (one stream
 * synchronise).  scratch: lograst_frustum_scratch_bytes(n). */
size_t lograst_frustum_scratch_bytes(int32_t n);
int lograst_frustum_select(int32_t n, int32_t num_points, const float* xyz, const int32_t* rows, const float* full_proj,
                           double padding, const float* scaling, const float* rotation, const float* opacity,
                           uint8_t* flag_out, int64_t* pos_out, int64_t* row_out, float* xyz_out, float* scaling_out,
                           float* rotation_out, float* opacity_out, void* scratch, size_t scratch_bytes, void* stream);
int lograst_frustum_read(const void* scratch, uint32_t* count_host, void* stream);

/* lograst_lod_select = the rest of LoG.prepare in one stream of launches and ONE read-back: (1) with root_weight given
 * (f32[num_roots], the root render's point_weight), root k is dropped unless root_weight[k] > 1e-8, and root_flag[root_pos[k]]
 * (u8[num_root_flags], the flag of lograst_frustum_select; root_pos = its pos_out) is cleared; (2) lograst_lod_traverse
 * from the remaining roots (root_rows i64[num_roots], the row_out above), same order and result, into out_index;
 * (3) a stable partition of out_index into out_leaf / out_node (capacity out_capacity each) by
 * opt_all_levels ? node_index[i] == -1 && depth[i] > 0 : depth[i] == current_depth (depth: i8[num_points]).
 * lograst_lod_select_read synchronises and returns the size of out_index, the size of out_leaf, and overflow /
 * frontier_left as lograst_lod_read does.  scratch: lograst_lod_select_scratch_bytes(...). */
size_t lograst_lod_select_scratch_bytes(int32_t num_roots, int32_t num_nodes, int32_t max_child, uint32_t out_capacity);
int lograst_lod_select(int32_t num_points, int32_t num_nodes, int32_t max_child, const int32_t* node_index,
                       const int32_t* tree, const int8_t* depth, const float* xyz, const float* scaling,
                       const float* rotation, const int64_t* root_rows, int32_t num_roots, const float* root_weight,
                       const int64_t* root_pos, uint8_t* root_flag, int32_t num_root_flags, const float* projmatrix,
                       const float* viewmatrix, float focal_x, float focal_y, float tanfovx, float tanfovy,
                       float min_resolution_pixel, int32_t levels, int32_t opt_all_levels, int32_t current_depth,
                       int64_t* out_index, uint32_t out_capacity, int64_t* out_leaf, int64_t* out_node, void* scratch,
                       size_t scratch_bytes, void* stream);
int lograst_lod_select_read(const void* scratch, uint32_t* count_all_host, uint32_t* count_leaf_host,
                            uint32_t* overflow_host, uint32_t* frontier_left_host, void* stream);

/* lograst_clamp_scale = LoG.clamp_scale on the rows index[i] (i64[m], unique, as for lograst_counter_update) with
 * flag[i] != 0 (u8[m]; NULL: all): scaling[r, :] = clamp(scaling[r, :], logf(radius3d_min[r]), logf(radius3d_max[r])) in
 * torch.clamp's order -- min > max gives log(max); a NaN in the value, the lower or the upper bound (in that order) is
 * the result.  Other rows, and rows outside [0, num_points), are not written. */
int lograst_clamp_scale(int32_t m, const int64_t* index, const uint8_t* flag, int32_t num_points, float* scaling,
                        const float* radius3d_min, const float* radius3d_max, void* stream);

/* lograst_init_radius3d = the initialisation pass, LoG.init with Gaussian.init_radius3d
 * (/root/reference/LoG/model/level_of_gaussian.py:328-332, :55-63) over ALL p points and `num_views` cameras in one launch.
 * xyz [p, 3], scaling [p, 3] and rotation [p, 4] are the RAW parameters: the kernel applies exp and normalize as
 * lograst_lod_traverse does.  cameras (device): num_views x 36 floats -- projmatrix[16], viewmatrix[16], focal_x, focal_y,
 * tanfovx, tanfovy, the arguments of lograst_compute_radius.  Per point and camera, in order: r = the radius of
 * lograst_compute_radius; where r > 0: r3d = exp(scaling[i, 0]) * (3.f / r) and radius3d_min[i] = minimum(radius3d_min[i],
 * r3d) as torch.minimum has it (a NaN on either side stays).  A row that no camera sees keeps its bits.  The minimum does
 * not depend on the order or the grouping of the cameras.
 * radius3d_min: in/out f32[p], or NULL.  valid (u8[p]: r > 0) and radius3d (f32[p]: r3d, exp(scaling[i, 0]) where r <= 0)
 * are Gaussian.init_radius3d's results, or NULL; they need num_views == 1.  p == 0 or num_views == 0: nothing happens. */
int lograst_init_radius3d(int32_t p, const float* xyz, const float* scaling, const float* rotation, int32_t num_views,
                          const float* cameras, float* radius3d_min, uint8_t* valid, float* radius3d, void* stream);

/* ---- "next" row N4: what LoG does with the rasterizer's outputs after every view ----------------------------
 * (a) lograst_id_histogram replaces `torch.unique(point_id_pixel, sorted=True, return_counts=True)` + dropping the
 *     leading -1 (/root/reference/LoG/render/renderer.py:156-159): ids_out (i32) = the distinct ids >= 0 in
 *     ascending order, counts_out (i64) = pixels each one wins; both need capacity min(n, num_pixels), n = number
 *     of Gaussians handed to the rasterizer (ids are < n).  The number of distinct ids stays on the device:
 *     lograst_id_histogram_read synchronises the stream and returns it.
 *     scratch: lograst_id_histogram_scratch_bytes(n). */
size_t lograst_id_histogram_scratch_bytes(int32_t n);
int lograst_id_histogram(int32_t n, const int32_t* point_id_pixel, int32_t num_pixels, int32_t* ids_out,
                         int64_t* counts_out, void* scratch, size_t scratch_bytes, void* stream);
int lograst_id_histogram_read(const void* scratch, uint32_t* count_host, void* stream);

/* (b) lograst_counter_update replaces Counter.update_by_output for ONE view
 *     (/root/reference/LoG/model/counter.py:36-68; caller LoG.update_by_output, level_of_gaussian.py:364-365).
 *     visible_index i64[nv] (no duplicates) maps the view's submitted Gaussians to model rows; grad_means2d
 *     f32[nv,3] is viewspace_points.grad; radii i32[nv]; point_weight f32[nv]; point_id i32[k] / point_count i64[k]
 *     the lists of (a).  The eight Counter buffers (length num_points, dtypes as registered at counter.py:7-19)
 *     are updated in place.  flag_vis_out (u8[nv], optional) receives radii > 0 (counter.py:48,50). */
int lograst_counter_update(int32_t nv, const int64_t* visible_index, const float* grad_means2d, const int32_t* radii,
                           const float* point_weight, int32_t k, const int32_t* point_id, const int64_t* point_count,
                           int32_t num_points, float* weights_max, float* weights_sum, float* grad_sum,
                           int16_t* radii_max, int16_t* visible_count, int32_t* radii_max_max, int32_t* area_sum,
                           int32_t* create_steps, uint8_t* flag_vis_out, void* stream);

/* (c) lograst_sparse_adam replaces SparseOptimizer.step + _single_tensor_adam
 *     (/root/reference/LoG/model/sparse_optimizer.py:41-78,163-196; caller LoG.step, level_of_gaussian.py:379-390):
 *     for every r < m with flag_vis[r] != 0 and every key, Adam on model row index[r] starting from the gathered
 *     parameter row r, with the reference's scalars: step_size = lr / (1 - beta1^step), bias_correction2_sqrt =
 *     sqrt(1 - beta2^step), eps; amsgrad when max_exp_avg_sq != NULL.  All keys go in one launch (num_keys <= 8). */
typedef struct lograst_adam_key {
  void* model_param;        /* f32 [num_points, width]: rows index[flag_vis] are rewritten */
  const void* param;        /* f32 [m, width]: params[key].data */
  const void* grad;         /* f32 [m, width]: params[key].grad */
  void* exp_avg;            /* f32 [num_points, width] */
  void* exp_avg_sq;         /* f32 [num_points, width] */
  void* max_exp_avg_sq;     /* f32 [num_points, width] or NULL */
  int32_t width;            /* floats per row */
  float step_size;          /* lr / bias_correction1 */
} lograst_adam_key;
int lograst_sparse_adam(int32_t m, int32_t num_points, const int64_t* index, const uint8_t* flag_vis,
                        int32_t num_keys, const lograst_adam_key* keys, double beta1, double beta2,
                        double bias_correction2_sqrt, double eps, void* stream);

/* Version 4: lograst_activate_backward (below) and lograst_sparse_adam in ONE launch, for steps of a single view (the
 * reference's trainer: one backward, then SparseOptimizer.step).  For every r < n with radii[r] > 0 (LoG's flag_vis,
 * LoG/model/counter.py:48) the raw gradients of row r are computed as lograst_activate_backward computes them (dl_dact_xyz
 * passes through) and applied at once to model row index[r] and its moments as lograst_sparse_adam applies them -- the
 * gradients are never written.  keys[6] in the order xyz, scaling, opacity, rotation, colors, shs (widths 3, 3, 1, 4, 3,
 * 3 * sh_coeffs; `grad` is ignored, `param` = the gathered raw rows [n, width]; model_param == NULL: key not optimised).
 * Same op sequences as the two kernels: the model and the moments come out bit for bit the same.
 * Alignment: raw_rotation and dl_dact_rotation must be 16-byte aligned (LOGRAST_ERR_ARG otherwise, before any device
 * work); every other pointer, the keys' blocks included, needs the alignment of its element type only. */
int lograst_activate_backward_adam(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                                   const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                                   const float* camera_center, const float* dl_dact_xyz, const float* dl_dact_scaling,
                                   const float* dl_dact_opacity, const float* dl_dact_rotation, const float* dl_dact_colors,
                                   int32_t num_points, const int64_t* index, const int32_t* radii,
                                   const lograst_adam_key* keys, double beta1, double beta2, double bias_correction2_sqrt,
                                   double eps, void* stream);

/* ---- steps over several views of the LoG model (Python side: log_amd/multi_view.py) ------------------------------------
 * The reference steps over ONE view: LoG.get_all writes visibility_flag['params'] per view and LoG.step reads the last
 * (level_of_gaussian.py:262-296, :379-398).  Here every view's activation backward is added into sums laid out by MODEL
 * row, and one Adam step is taken over the rows some view saw.  Neither call allocates; all work on `stream`.
 *
 * A target is one key's block of per-model-row sums: row p starts at base + p * row_stride_floats.  The attribute-major
 * blocks of log_amd.dist have row_stride_floats = the key's width; its row-major form is 16-float rows with the key's first
 * column as `base` (and a separate shs block).  base == NULL: the key is not accumulated.  Offsets are 64-bit:
 * lograst_accumulate_target_floats(num_points, row_stride_floats, width) = the floats such a block spans
 * ((num_points - 1) * row_stride_floats + width, 0 for no rows; computed as the kernels compute an element's offset). */
typedef struct lograst_acc_target {
  float* base;
  int32_t row_stride_floats;
} lograst_acc_target;
size_t lograst_accumulate_target_floats(int32_t num_points, int32_t row_stride_floats, int32_t width);

/* For every r < n with radii[r] > 0 and 0 <= index[r] < num_points: the raw gradients of row r exactly as
 * lograst_activate_backward computes them (same op sequences; dl_dact_xyz passes through; coefficients above the active
 * degree get zero) are ADDED into row index[r] of targets[6] (order xyz, scaling, opacity, rotation, colors, shs; widths 3,
 * 3, 1, 4, 3, 3 * sh_coeffs; row_stride_floats >= width) and seen[index[r]] (i32[num_points]) is incremented.  Other rows
 * are not written.  Plain read-modify-writes, no atomics: index (i64[n]) has no duplicates (the contract of
 * lograst_counter_update) and the views follow each other on the stream, so the same views in the same order give the same
 * bits: after each view a sum is fp32(sum + gradient). */
int lograst_activate_backward_accumulate(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                                         const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                                         const float* camera_center, const float* dl_dact_xyz, const float* dl_dact_scaling,
                                         const float* dl_dact_opacity, const float* dl_dact_rotation,
                                         const float* dl_dact_colors, int32_t num_points, const int64_t* index,
                                         const int32_t* radii, const lograst_acc_target* targets, int32_t* seen,
                                         void* stream);

/* For every row p < num_points with seen[p] > 0: Adam on model row p and its moments with the op sequence and the scalars
 * of lograst_sparse_adam -- given the same gradient bits, the same result bits; amsgrad where max_exp_avg_sq != NULL -- then
 * the row's accumulated gradient is overwritten with zeros, seen[p] = 0 and moved_out[p] = 1 (u8[num_points], or NULL).
 * Rows with seen[p] == 0 get moved_out[p] = 0; nothing else of theirs is read or written.  keys[6] in the order and with the
 * widths above: model_param is updated in place, `param` is ignored, `grad` is the key's accumulated block with rows
 * grad_row_stride_floats[key] apart; model_param == NULL skips the key. */
int lograst_accumulated_adam(int32_t num_points, int32_t* seen, const lograst_adam_key* keys,
                             const int32_t* grad_row_stride_floats, double beta1, double beta2,
                             double bias_correction2_sqrt, double eps, uint8_t* moved_out, void* stream);

/* ---- densification: TensorTree.split_and_remove + Splitter.split_and_remove(_other) on the device ----------------
 * (LoG/model/tensor_tree.py:65-129, LoG/model/splitter.py:5-31, :95-220).  One call of the reference method is:
 * lograst_densify_plan, lograst_densify_read (the only host synchronisation: the caller allocates the new buffers from
 * the counts), lograst_densify_src_rows, then lograst_densify_move_rows / _split_uniform / _tree as the method needs.
 * children = the tree's max_child = Splitter.N, one of 2, 4, 8.  No call allocates; all work on `stream`.
 *
 * lograst_densify_plan: flag_split / flag_remove u8[p] (torch bool).  With node_index (i32[p]), index_parent (i32[p]) and
 * depth (i8[p]) given (all three or none) the tree's masks are applied first: remove &= leaf & ~root, split &= leaf &
 * depth < max_level.  split_out / remove_out u8[p] receive the masked flags (not the inputs' storage).  A row is kept
 * unless it is removed, or split while remove_split != 0.  keep_dest i32[p] = the new row of a kept row, -1 otherwise.
 * The scratch header then holds num_keep, num_split and overlap = rows flagged for both while remove_split == 0 (the
 * reference leaves that case undefined: callers fall back).  scratch: lograst_densify_scratch_bytes(p), kept until
 * lograst_densify_src_rows has run. */
size_t lograst_densify_scratch_bytes(int32_t p);
int lograst_densify_plan(int32_t p, const uint8_t* flag_split, const uint8_t* flag_remove, int32_t remove_split,
                         int32_t children, const int32_t* node_index, const int32_t* index_parent, const int8_t* depth,
                         int32_t max_level, uint8_t* split_out, uint8_t* remove_out, int32_t* keep_dest, void* scratch,
                         size_t scratch_bytes, void* stream);
/* Synchronises the stream and returns the three counts. */
int lograst_densify_read(const void* scratch, uint32_t* num_keep_host, uint32_t* num_split_host, uint32_t* overlap_host,
                         void* stream);
/* src_row i32[num_keep + children * num_split]: new row d < num_keep came from old row src_row[d]; new row
 * num_keep + children * k + j is child j of the k-th split row (ascending old index), src_row = that row.
 * split / remove: the masked flags of the plan; num_keep / num_split: what lograst_densify_read returned. */
int lograst_densify_src_rows(int32_t p, int32_t children, int32_t remove_split, const uint8_t* split, const uint8_t* remove,
                             int32_t num_keep, int32_t num_split, int32_t* src_row, const void* scratch, void* stream);

/* lograst_densify_move_rows: dst[d] = src[src_row[d]] for up to 8 keys in one launch, 16-byte stores throughout and
 * 16-byte loads where the row size allows.  Rows d >= num_keep follow child_mode.  dst must be 16-byte aligned and src
 * aligned to elem_size; both contiguous.  Rows d >= num_keep of a LOGRAST_MOVE_SKIP key are not written here: they are
 * unspecified until the kernel that owns the children has run. */
#define LOGRAST_MOVE_COPY_PARENT 0
#define LOGRAST_MOVE_ZERO 1
#define LOGRAST_MOVE_SKIP 2      /* another kernel writes the children (lograst_densify_split_uniform) */
typedef struct lograst_move_key {
  const void* src;          /* [src_rows, columns] of elem_size bytes */
  void* dst;                /* [num_new, columns] */
  int32_t elem_size;        /* 1, 2 or 4 */
  int32_t columns;          /* elements per row, elem_size * columns <= 65536 */
  int32_t child_mode;       /* LOGRAST_MOVE_* */
} lograst_move_key;
int lograst_densify_move_rows(int32_t num_keep, int32_t num_new, int32_t src_rows, const int32_t* src_row,
                              int32_t num_keys, const lograst_move_key* keys, void* stream);

/* split_by_uniform (splitter.py:95-130): rows num_keep.. of xyz_new f32[num_new, 3] and scaling_new f32[num_new, 3] (raw
 * log-scales) from the old xyz / scaling (raw) / rotation (raw quaternion, normalised inside) rows src_row names:
 * log2(children) rounds, each halving the longest CURRENT axis (ties: lowest axis) by scaling_factor and moving the two
 * halves +-0.5 * scale[axis] along that axis.  Child order: parent-major, then (--, -+, +-, ++). */
int lograst_densify_split_uniform(int32_t num_keep, int32_t num_split, int32_t children, float scaling_factor,
                                  int32_t src_rows, const int32_t* src_row, const float* xyz, const float* scaling,
                                  const float* rotation, float* xyz_new, float* scaling_new, void* stream);

/* The tree buffers that TensorTree.split followed by TensorTree.remove leave (tensor_tree.py:65-118): node_index_new,
 * index_parent_new i32[num_new], local_index_new, depth_new i8[num_new], tree_new i32[num_nodes + num_split, children];
 * split = the plan's masked split flags (remove_split = 0), keep_dest its output. */
int lograst_densify_tree(int32_t p, int32_t num_nodes, int32_t children, int32_t num_keep, int32_t num_split,
                         const int32_t* src_row, const int32_t* keep_dest, const uint8_t* split, const int32_t* node_index,
                         const int32_t* index_parent, const int8_t* local_index, const int8_t* depth, const int32_t* tree,
                         int32_t* node_index_new, int32_t* index_parent_new, int8_t* local_index_new, int8_t* depth_new,
                         int32_t* tree_new, void* stream);

/* ---- rows N2 / N3: LoG.get_all + Activation.activate_root_return, fused ---------------------------------------
 * Replaces the per-key gathers of LoG.get_all (/root/reference/LoG/model/level_of_gaussian.py:262-296) and the
 * activations of Activation.activate_root_return / colors_activation (/root/reference/LoG/model/activation.py:27-44;
 * SH polynomial /root/reference/LoG/model/sh_utils.py:31-72).  For every r < n, row index[r] of the model buffers
 * (xyz[P,3], scaling[P,3] log-scales, opacity[P,1] logits, rotation[P,4], colors[P,3] SH DC term, shs[P,K,3] higher
 * coefficients, K = 0 allowed with shs = NULL) is copied to the raw_* outputs [n, ...] (the step's parameters) and
 * activated: act_scaling = exp, act_opacity = sigmoid, act_rotation = q / max(|q|, 1e-12), act_colors =
 * 0.28209479 * colors + 0.5 (+ eval_sh_wobase(normalize(xyz - camera_center), shs, active_degree) when
 * active_degree > 0; degrees 1..3, camera_center = 3 floats on the device).  xyz is passed through (raw_xyz).
 * An index[r] below 0 or >= num_points reads row 0 of the model.
 * Alignment: rotation, raw_rotation and act_rotation are read and written one quaternion (16 bytes) at a time and must be
 * 16-byte aligned (LOGRAST_ERR_ARG otherwise, before any device work); every other pointer, shs and raw_shs included,
 * needs 4 bytes (index: 8). */
int lograst_gather_activate(int32_t n, int32_t num_points, const int64_t* index, const float* xyz,
                            const float* scaling, const float* opacity, const float* rotation, const float* colors,
                            const float* shs, int32_t sh_coeffs, int32_t active_degree, const float* camera_center,
                            float* raw_xyz, float* raw_scaling, float* raw_opacity, float* raw_rotation,
                            float* raw_colors, float* raw_shs, float* act_scaling, float* act_opacity,
                            float* act_rotation, float* act_colors, void* stream);
/* Backward of the activations for the first n rows (the rows that are parameters): from dL/d(act_*) to
 * dL/d(raw_*).  dl_dshs (may be NULL) is [n, sh_coeffs, 3]; coefficients above active_degree get 0.  The direction
 * is detached in the reference (activation.py:30), so xyz receives no gradient from the colours.
 * Alignment: raw_rotation, dl_dact_rotation and dl_drotation must be 16-byte aligned (LOGRAST_ERR_ARG otherwise, before
 * any device work).  dl_dshs needs 4 bytes: it is written 16 bytes at a time when 3 * sh_coeffs % 4 == 0 and it is 16-byte
 * aligned, one float at a time otherwise, with the same bits.  Every other pointer: 4 bytes. */
int lograst_activate_backward(int32_t n, const float* raw_xyz, const float* raw_scaling, const float* raw_opacity,
                              const float* raw_rotation, int32_t sh_coeffs, int32_t active_degree,
                              const float* camera_center, const float* dl_dact_scaling, const float* dl_dact_opacity,
                              const float* dl_dact_rotation, const float* dl_dact_colors, float* dl_dscaling,
                              float* dl_dopacity, float* dl_drotation, float* dl_dcolors, float* dl_dshs, void* stream);

/* ---- the photometric training loss (LoG/render/renderer.py:253-266 calculate_loss, LoG/render/loss.py:6-44 SSIM) ----
 * For render, render_l1, gt of shape [batch, channels, height, width], fp32, each addressed through FOUR ELEMENT STRIDES
 * (b, c, y, x; host arrays of 4 int64 -- a channels-last view is read in place):
 *   ssim = 1 - mean(ssim_map(render, gt))   11x11 Gaussian window (sigma 1.5, taps normalised in double and rounded to
 *                                           fp32 once, applied separably), no padding: (height-10) x (width-10) outputs,
 *                                           C1 = 0.01^2, C2 = 0.03^2
 *   l1   = mean |render_l1 - gt|            render_l1 == NULL: render itself (LoG passes its colour-corrected render here)
 *   loss = ssim_weight * ssim + l1_weight * l1
 * lograst_loss_forward writes out3 = (loss, l1, ssim) on the device and, for the backward, maps: 3 * batch * channels *
 * (height-10) * (width-10) floats (the derivatives of the loss's SSIM term with respect to the window mean of render and
 * the two window second moments that contain render; NULL: forward only).  The two sums are reduced from per-workgroup
 * partials (scratch: lograst_loss_scratch_bytes) in a fixed order: the same input gives the same bits.
 * lograst_loss_backward reads the upstream gradient of loss from DEVICE memory (grad_loss, one float) and writes
 * grad_render [batch, channels, height, width] (contiguous); the L1 term goes to grad_render_l1 (contiguous, same shape)
 * when render_l1 != NULL and into grad_render otherwise; sign(0) = 0.  gt gets no gradient.
 * height < 11 or width < 11 is an error; batch * channels == 0 writes zeros to out3 and launches nothing. */
size_t lograst_loss_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width);
int lograst_loss_forward(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                         const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                         const float* gt, const int64_t* gt_strides, float ssim_weight, float l1_weight, float* out3,
                         float* maps, void* scratch, size_t scratch_bytes, void* stream);
int lograst_loss_backward(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                          const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                          const float* gt, const int64_t* gt_strides, float l1_weight, const float* grad_loss,
                          const float* maps, float* grad_render, float* grad_render_l1, void* stream);

/* The same loss with the L1 term on a per-image channel gain (LoG's view correction, renderer.py:243-245, without its
 * render_correct tensor): l1 = mean | l1_gain[b, c] * render[b, c, y, x] - gt |, l1_gain fp32 [batch, channels] on the
 * device, contiguous; the SSIM term is on render as above.  The product is one fp32 multiply and the subtraction a
 * separate operation, so sign(0) = 0 holds exactly where gt == fp32(gain * render).
 * lograst_loss_backward_gain writes ONE image gradient, grad_render = SSIM part + gain * (grad_loss * l1_scale * sign),
 * and grad_gain[batch, channels] = grad_loss * l1_scale * sum over the plane of sign(gain * render - gt) * render,
 * l1_scale = l1_weight / (batch * channels * height * width): per-workgroup sums in double, added per plane in a fixed
 * order in double (scratch) and rounded to fp32 once -- no floating-point atomics, the same bits from run to run.
 * scratch: lograst_loss_gain_scratch_bytes bytes, 8-byte aligned, serves either call. */
size_t lograst_loss_gain_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width);
int lograst_loss_forward_gain(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                              const int64_t* render_strides, const float* gt, const int64_t* gt_strides, const float* l1_gain,
                              float ssim_weight, float l1_weight, float* out3, float* maps, void* scratch, size_t scratch_bytes,
                              void* stream);
int lograst_loss_backward_gain(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                               const int64_t* render_strides, const float* gt, const int64_t* gt_strides, const float* l1_gain,
                               float l1_weight, const float* grad_loss, const float* maps, float* grad_render, float* grad_gain,
                               void* scratch, size_t scratch_bytes, void* stream);

/* The same loss with masks (LoG/render/renderer.py:253-266 calculate_loss with mask_ignore, :343-370 MaskForeground):
 * mask, foreground: fp32 [batch, height, width], each through THREE ELEMENT STRIDES (b, y, x), either may be NULL but
 * not both (without masks use the entry points above).  Per image element, one fp32 operation each and in this order:
 *   g = gt * f + (1 - f) * background[c]      with foreground (background: fp32 [channels] on the device); else g = gt
 *   x = g * m + render * (1 - m)              with mask; else x = render
 *   ssim = 1 - mean(ssim_map(x, g));  l1 = mean |x - g|, or |render_l1 - g|, or |l1_gain[b, c] * render - g| (render_l1 and
 *   l1_gain exclude each other and read the PLAIN render, as the reference's render_correct does); the means are over
 *   all elements -- nothing is renormalised by a mask.
 * With foreground, gt_out [batch, channels, height, width] (contiguous) receives g and is REQUIRED: it is the gt of the
 * backward.  lograst_loss_backward_masked takes that composited gt (or the caller's gt without foreground) and the mask
 * (without a mask the plain backward entry points on the composited gt are the backward): grad_render = (1 - m) * (SSIM
 * part + L1 part) when the L1 term reads x; (1 - m) * SSIM part with render_l1 (grad_render_l1 = L1 part) and
 * (1 - m) * SSIM part + gain * L1 part with l1_gain (grad_gain as lograst_loss_backward_gain).  Masks, foreground and
 * background get no gradient.  scratch: lograst_loss_masked_scratch_bytes, 8-byte aligned, serves either call (the
 * backward reads it only with l1_gain). */
size_t lograst_loss_masked_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width);
int lograst_loss_forward_masked(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                                const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                                const float* gt, const int64_t* gt_strides, const float* l1_gain, const float* mask,
                                const int64_t* mask_strides, const float* foreground, const int64_t* foreground_strides,
                                const float* background, float* gt_out, float ssim_weight, float l1_weight, float* out3,
                                float* maps, void* scratch, size_t scratch_bytes, void* stream);
int lograst_loss_backward_masked(int32_t batch, int32_t channels, int32_t height, int32_t width, const float* render,
                                 const int64_t* render_strides, const float* render_l1, const int64_t* render_l1_strides,
                                 const float* gt, const int64_t* gt_strides, const float* l1_gain, const float* mask,
                                 const int64_t* mask_strides, float l1_weight, const float* grad_loss, const float* maps,
                                 float* grad_render, float* grad_render_l1, float* grad_gain, void* scratch, size_t scratch_bytes,
                                 void* stream);

/* The bounding box of a foreground mask (MaskForeground.bound_from_mask, renderer.py:319-326) in one pass: mask fp32
 * [batch, height, width] through three element strides; record (lograst_mask_bounds_bytes, 4-byte aligned) receives per
 * image eight int32 {xmin, ymin, xmax, ymax, count, 0, 0, 0} over the pixels with mask > threshold (strict: a NaN is
 * not foreground); an image without such a pixel leaves {width, height, -1, -1, 0}.  The call initialises the record
 * itself on the same stream and allocates nothing; integer atomics only, so the result is exact and repeatable.
 * lograst_mask_bounds_read copies batch * 8 int32 to the host and synchronises the stream (the one synchronisation). */
size_t lograst_mask_bounds_bytes(int32_t batch);
int lograst_mask_bounds(int32_t batch, int32_t height, int32_t width, const float* mask, const int64_t* mask_strides,
                        float threshold, void* record, size_t record_bytes, void* stream);
int lograst_mask_bounds_read(const void* record, int32_t batch, int32_t* host_out, void* stream);

/* ---- Corrector.step (LoG/model/corrector.py:35-62): the AMSGrad step of ONE row of the view correction ----------------
 * steps i32[views]; param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq f32[views, width], contiguous, 1 <= width <= 64.
 * One launch of one wave: steps[index] += 1; s = steps[index] - start_step; s < 0: nothing else is touched (grad stays).
 * Otherwise t = clip(s / 100, 0, 1), lr = exp(log(lr_init) (1 - t) + log(lr_final) t) in double, the reference's
 * _single_tensor_adam with max_exp_avg_sq (betas 0.9 / 0.999, eps 1e-15, bias corrections 1 - beta^s in fp32, a maximum
 * that hands a NaN on) on the row, then grad[index] = 0.  Nothing comes back to the host; index is a host integer. */
int lograst_corrector_step(int32_t views, int32_t width, int32_t index, int32_t start_step, double lr_init, double lr_final,
                           int32_t* steps, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                           void* stream);

/* ---- a per-view pose table (log_amd/pose.py) ---------------------------------------------------------------------------
 * table f32[views, 6], contiguous: row i = (omega[3], upsilon[3]), the camera-frame perturbation p_cam' = R(omega) p_cam +
 * upsilon of view i, R by Rodrigues' formula (its series below |omega|^2 = 1e-2).  viewmatrix / projmatrix: [4, 4] fp32
 * device arrays in the rasterizer's row-vector convention.  With E = [[R^T - I, 0], [upsilon, 0]] and W = viewmatrix E:
 *   viewmatrix_out = viewmatrix + W,  projmatrix_out = projmatrix + W (viewmatrix^-1 projmatrix),
 *   campos_out [3] = row 3 of viewmatrix_out^-1,
 * both inverses by the rigid closed form, everything in double and rounded once: a zero row returns the inputs' bits.
 * lograst_pose_backward ADDS dL/d(row index) into table_grad f32[views, 6] from dL/dviewmatrix_out, dL/dprojmatrix_out and
 * dL/dcampos_out (each may be NULL = zeros; all NULL: nothing is launched); viewmatrix and projmatrix are constants.
 * One launch of one wave each, nothing comes back to the host; index is a host integer.  The table steps with
 * lograst_corrector_step at width 6. */
int lograst_pose_apply(int32_t views, int32_t index, const float* table, const float* viewmatrix, const float* projmatrix,
                       float* viewmatrix_out, float* projmatrix_out, float* campos_out, void* stream);
int lograst_pose_backward(int32_t views, int32_t index, const float* table, const float* viewmatrix, const float* projmatrix,
                          const float* dl_dviewmatrix, const float* dl_dprojmatrix, const float* dl_dcampos, float* table_grad,
                          void* stream);

/* ---- the depth term of depth-supervised training (LoG/render/renderer.py:268-292 append_depth_loss with
 * LoG/render/loss.py:47-117 ScaleAndShiftInvariantLoss, one gradient scale) --------------------------------------------
 * pred, gt, acc: [height, width] fp32, each addressed through TWO ELEMENT STRIDES (y, x; host arrays of 2 int64).
 * rows, cols: n int64 patch origins ON THE DEVICE (never read by the host); patches are 64 x 64, 1 <= n <= 256.
 * Per pixel m = acc > threshold, p = 1 / (pred + eps); per patch the least-squares (s, h) of s p + h onto gt over m
 * (s = h = 0 where the determinant is exactly 0), d = m (s p + h - gt);
 *   loss = (sum_k sum d^2 + alpha * sum_k sum_{horizontal and vertical neighbour pairs inside the patch} m m' |d' - d|) / M,
 *   M = the number of valid pixels over all patches (M == 0: loss = nan).
 * All arithmetic is double; sums run in a fixed order, so the same input gives the same bits.
 * lograst_depth_loss_forward writes out (16 bytes, 8-byte aligned: the loss as a float at byte 0, M as a double at byte 8)
 * and records (lograst_depth_loss_record_bytes(n) = 128 * (n + 1) bytes, 8-byte aligned: a header and one record of 16
 * doubles per patch), all the backward needs besides the three images.  A patch that does not lie inside the image is
 * not read: the loss becomes nan and the patch adds nothing to the gradient.
 * lograst_depth_loss_backward reads the upstream gradient of loss from DEVICE memory (grad_loss, one float) and writes
 * every element of grad_pred [height, width] (contiguous) once: scale and shift are not detached; pixels outside every
 * patch get 0.  gt and acc get no gradient.
 * height or width below 64, n outside 1..256, NULL pointers and too small a records buffer are errors. */
size_t lograst_depth_loss_record_bytes(int32_t n);
int lograst_depth_loss_forward(int32_t height, int32_t width, const float* pred, const int64_t* pred_strides,
                               const float* gt, const int64_t* gt_strides, const float* acc, const int64_t* acc_strides,
                               int32_t n, const int64_t* rows, const int64_t* cols, double alpha, double eps,
                               double threshold, void* out, void* records, size_t record_bytes, void* stream);
int lograst_depth_loss_backward(int32_t height, int32_t width, const float* pred, const int64_t* pred_strides,
                                const float* gt, const int64_t* gt_strides, const float* acc, const int64_t* acc_strides,
                                int32_t n, const void* records, const float* grad_loss, float* grad_pred, void* stream);

/* ---- evaluation: what a validation image costs after it is rendered (LoG/utils/trainer.py:313-332 make_validation,
 * LoG/utils/metric.py psnr and ssim, LoG/render/renderer.py:19-23 tensor_to_bgr) ----------------------------------------
 * Images are [channels, height, width] fp32, 1 <= channels <= 4, each addressed through THREE ELEMENT STRIDES (c, y, x;
 * host arrays of 3 int64, y and x strides not negative), so a view of an HWC image is read in place.
 * lograst_image_to_bgr8 writes out = uint8 [height, width, channels] (4-byte aligned), the channel order reversed, each
 * byte (uint8) trunc(fp32(min(max(x, 0), 1) * 255.f)): the bytes of tensor_to_bgr for every input that is not a nan.
 * lograst_eval_metrics: with LOGRAST_EVAL_FIT_GAIN, gain[c] = fp32(sum gt * pred / sum pred^2) over the columns
 * [0, width / 2) (double sums in a fixed order; nan or inf where the reference's division gives one) and
 * p = min(max(fp32(gain[c] * pred), 0), 1), a nan staying a nan; without it p = pred, not clamped.  d = p - gt.  The record
 * (128 bytes, 8-byte aligned, 16 doubles ON THE DEVICE) gets [0] sum |d|, [1] sum d^2, [2] with LOGRAST_EVAL_SSIM the sum of
 * the SSIM map of metric.py:33-103 over p and gt (11 taps, sigma 1.5, zero padding: height * width outputs per channel;
 * variances clamped at 0, the covariance limited to sqrt(s00 * s11); c1 = (0.01 max_val)^2, c2 = (0.03 max_val)^2), else 0,
 * [3] the element count, [4..7] gain (1 without the fit, 0 beyond `channels`), [8..11] sum gt * pred, [12..15] sum pred^2.
 * corrected (or NULL): fp32 [channels, height, width] contiguous, gets p.  bgr8 (or NULL): uint8 [2 * height, width,
 * channels], the 8-bit form (as lograst_image_to_bgr8) of p above gt, each byte of p converted from the value `corrected`
 * holds.  No floating-point atomics: the same input gives the same bits.
 * lograst_eval_read copies the record to the host and synchronises the stream: the one synchronisation.
 * NULL pointers, channels outside 1..4, height or width below 1, too small a scratch buffer, 2^31 elements or more and a
 * plane whose strides reach beyond 32-bit offsets are errors, reported before any device work. */
#define LOGRAST_EVAL_FIT_GAIN 1
#define LOGRAST_EVAL_SSIM 2
size_t lograst_eval_scratch_bytes(int32_t channels, int32_t height, int32_t width);
int lograst_image_to_bgr8(int32_t channels, int32_t height, int32_t width, const float* image, const int64_t* strides3,
                          uint8_t* out, void* stream);
int lograst_eval_metrics(int32_t channels, int32_t height, int32_t width, const float* pred, const int64_t* pred_strides3,
                         const float* gt, const int64_t* gt_strides3, int32_t flags, double max_val, float* corrected,
                         uint8_t* bgr8, void* record, void* scratch, size_t scratch_bytes, void* stream);
int lograst_eval_read(const void* record, double* out16, void* stream);

/* ---- densification decisions: LoG.update_depth_stage / update_init_stage up to the flags -------------------------
 * (LoG/model/level_of_gaussian.py:400-427, :454-508).  One event is: lograst_decide_depth or lograst_decide_init (the
 * flags, every count and statistic the reference logs and, for the depth stage, the top-k cut, all on `stream`), then
 * lograst_decide_read -- the only host synchronisation -- and, after the caller has resized the model with the flags,
 * lograst_decide_child_radius_max.  No call allocates.  p = 0 is legal.
 *
 * A statistic is what Counter.str_min_mean_max prints of a population x (fp32): count, min, max (NaN if any x is NaN)
 * and the sums of x and x * x in double, from which mean = sum / count and the unbiased std =
 * sqrt((sumsq - sum * sum / count) / (count - 1)).  The sums are formed per workgroup and combined in a fixed order by one
 * workgroup, without floating-point atomics: the same inputs give the same bits.  count == 0: min = +inf, max = -inf. */
typedef struct lograst_decide_stat {
  double sum, sumsq;
  float min, max;
  uint32_t count, reserved;
} lograst_decide_stat;

#define LOGRAST_DECIDE_DEPTH_BINS 256   /* bin = depth + 128 (depth is int8) */
/* counts[] of the depth stage */
#define LOGRAST_DECIDE_SPLIT_GRAD 0     /* rows with grad > split_grad_thres */
#define LOGRAST_DECIDE_SPLIT_RADII 1    /* rows with radii_max_max > radius2d_thres */
#define LOGRAST_DECIDE_CANDIDATES 2     /* rows of flag_split before the cut */
#define LOGRAST_DECIDE_REMOVED 3        /* rows of flag_remove */
#define LOGRAST_DECIDE_DEPTH_LT 4       /* rows with depth < current_depth */
/* counts[] of the init stage */
#define LOGRAST_DECIDE_REMOVE_WEIGHT 0  /* weights_max < init_weight_min */
#define LOGRAST_DECIDE_NONMAX 1         /* weights_max < sigmoid(opacity) * 0.1 */
#define LOGRAST_DECIDE_REMOVE_SMALL 2   /* radii_max_max < small_thres, before the random half is taken */
#define LOGRAST_DECIDE_INIT_SPLIT_GRAD 3
#define LOGRAST_DECIDE_INIT_SPLIT_RADII 4
typedef struct lograst_decide_record {
  uint32_t counts[8];
  /* the cut (depth stage): num_max_split = min(int(fp32(counts[DEPTH_LT]) * 0.05f), max_split_points); need_cut =
   * counts[CANDIDATES] > num_max_split.  With need_cut and num_max_split > 0, cut_value is the num_max_split-th largest
   * radii_max_max among the candidates, cut_thres = (float)cut_value, and flag_split keeps the candidates with
   * (float)radii_max_max >= cut_thres (ties stay).  With need_cut and num_max_split == 0 no cut is applied (the
   * reference raises there: callers fall back). */
  uint32_t need_cut, num_max_split;
  int32_t cut_value;
  float cut_thres;
  uint32_t depth_all[LOGRAST_DECIDE_DEPTH_BINS];      /* every row, by depth */
  uint32_t depth_split[LOGRAST_DECIDE_DEPTH_BINS];    /* rows of the final flag_split with depth < max_level */
  uint32_t depth_remove[LOGRAST_DECIDE_DEPTH_BINS];   /* rows of flag_remove */
  /* depth stage: opacity, ratio, grad, radii over the is_parent rows.  init stage: radii_max over the activated rows,
   * grad over all rows, radii_max over the rows of flag_split, radius3d_min as it will be after the resize (rows that are
   * neither split nor removed once, split rows `children` times). */
  lograst_decide_stat stats[4];
} lograst_decide_record;

/* lograst_decide_depth.  Per row i < p:
 *   grad      = grad_sum / (float)max(area_sum, 1)                      (one correctly rounded fp32 division)
 *   is_parent = node_index == -1 && depth < current_depth
 *   remove    = node_index == -1 && depth > 0 && weights_max < remove_weights_thres && visible_count > 1
 *   split     = grad > split_grad_thres && (float)radii_max_max > radius2d_thres && is_parent &&
 *               create_steps > min_steps_split && !remove,   then the cut (lograst_decide_record).
 * opacity = 1 / (1 + expf(-raw)), ratio = max / (((e0 + e1) + e2) - max - min) of e = expf(scaling): the expressions of
 * lograst_gather_activate.  flag_split / flag_remove: u8[p] (torch bool), written for every row. */
typedef struct lograst_decide_depth_args {
  const float* opacity;            /* f32 [p] raw (column 0 of [p, 1]) */
  const float* scaling;            /* f32 [p, 3] raw */
  const int32_t* node_index;       /* i32 [p] */
  const int8_t* depth;             /* i8  [p] */
  const int32_t* create_steps;     /* i32 [p] */
  const float* grad_sum;           /* f32 [p] */
  const int32_t* area_sum;         /* i32 [p] */
  const int32_t* radii_max_max;    /* i32 [p] */
  const float* weights_max;        /* f32 [p] */
  const int16_t* visible_count;    /* i16 [p] */
  int32_t current_depth, max_level, min_steps_split, max_split_points;
  float split_grad_thres, radius2d_thres, remove_weights_thres;
  uint8_t* flag_split;             /* out u8 [p] */
  uint8_t* flag_remove;            /* out u8 [p] */
} lograst_decide_depth_args;

/* lograst_decide_init (init_split_method 'split_by_2d').  Per row:
 *   remove     = weights_max < init_weight_min || weights_max < sigmoid(opacity) * 0.1f ||
 *                ((float)radii_max_max < small_thres && rand > 0.5f)
 *   activation = create_steps > min_steps && radii_max_max > 0
 *   split      = activation && ((float)radii_max_max > split_thres_sq ||
 *                (grad > grad_thres && (float)radii_max_max > radius_thres)) && !remove
 * The caller forms the thresholds from the configuration in double, as Python does, and narrows them once. */
typedef struct lograst_decide_init_args {
  const float* opacity;            /* f32 [p] raw */
  const int32_t* create_steps;     /* i32 [p] */
  const float* grad_sum;           /* f32 [p] */
  const int32_t* area_sum;         /* i32 [p] */
  const int32_t* radii_max_max;    /* i32 [p] */
  const float* weights_max;        /* f32 [p] */
  const float* rand;               /* f32 [p]: torch.rand_like(weights_max) */
  const float* radius3d_min;       /* f32 [p] */
  int32_t min_steps, children;
  float init_weight_min;           /* init_weight_min */
  float small_thres;               /* (init_radius_min * scale) ** 2 */
  float split_thres_sq;            /* (init_radius_split * scale) ** 2 */
  float grad_thres;                /* 10 * split_grad_thres */
  float radius_thres;              /* init_radius_min * scale * 8 */
  uint8_t* flag_split;             /* out u8 [p] */
  uint8_t* flag_remove;            /* out u8 [p] */
} lograst_decide_init_args;

/* scratch: lograst_decide_scratch_bytes(p) bytes, 16-byte aligned, uninitialised, kept until lograst_decide_read. */
size_t lograst_decide_scratch_bytes(int32_t p);
int lograst_decide_depth(int32_t p, const lograst_decide_depth_args* args, void* scratch, size_t scratch_bytes, void* stream);
int lograst_decide_init(int32_t p, const lograst_decide_init_args* args, void* scratch, size_t scratch_bytes, void* stream);
/* Copies the record of the last lograst_decide_depth / _init on this scratch to the host and synchronises the stream.
 * record_bytes must be sizeof(lograst_decide_record). */
int lograst_decide_read(const void* scratch, lograst_decide_record* record_host, size_t record_bytes, void* stream);
/* After the resize of a depth-stage event (the split rows stay, their children are the last num_children rows):
 * radius3d_max[j] = scaling_decay * max(expf(scaling[index_parent[j]])) for the rows j >= num_points - num_children
 * (level_of_gaussian.py:516-519).  index_parent i32[num_points], scaling f32[num_points, 3], radius3d_max
 * f32[num_points]; a row whose parent is out of range is left alone. */
int lograst_decide_child_radius_max(int32_t num_points, int32_t num_children, const int32_t* index_parent,
                                    const float* scaling, float scaling_decay, float* radius3d_max, void* stream);

/* ---- per-kernel timing with HIP events on the launch stream (used by bench.py) -----------------
 * When enabled every kernel launch is bracketed by hipEventRecord on its stream.  read() synchronises
 * the recorded events and returns, for kernel slot i < LOGRAST_NUM_KERNELS, accumulated milliseconds
 * and launch counts since the last reset. */
#define LOGRAST_NUM_KERNELS 23   /* 22 + "recolor" (lograst_recomposite), appended within version 4 */
void lograst_profile_enable(int on);
void lograst_profile_reset(void);
int lograst_profile_read(double* ms_out, int64_t* count_out);
const char* lograst_kernel_name(int slot);

#ifdef __cplusplus
}
#endif
#endif /* LOGRAST_H */
