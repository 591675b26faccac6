// prepare.hip -- what LoG does around the level-of-detail traversal for every view, and after every optimizer step
// (/root/reference/LoG/model/level_of_gaussian.py):
//   * frustum selection (Gaussian._visible_flag_by_camera :39-53 + the boolean-mask indexing of LoG.prepare :227-240 and
//     Gaussian.prepare :90-98): flag, the positions of the kept entries, their rows and -- for the root render of
//     LoG.prepare -- their activated parameters, compacted in order;
//   * the root filter by the root render's point_weight (:241-242) and the leaf / node partition of the selected list
//     (:244-251), either side of the traversal of lod.hip;
//   * LoG.clamp_scale (:367-377) on the rows an (index, flag) pair selects.
// Compaction is lod.hip's: per-1024-entry counts, one workgroup scans the counts (any number of chunks, 1024 a round),
// ballot ranks inside the chunk -- stable, no atomics, no dependence on the order workgroups run in.
#include "common.hpp"
#include "launch.hpp"

#define PREP_CHUNK 1024u

// rank of every set entry of a chunk in slot order (k, wave, lane): call with the four predicates of a thread
struct PrepRank {
  uint64_t b[4];
  uint32_t before[4];   // set entries of this chunk in front of (k, wave)
};
LR_DEV void prep_rank(const bool set[4], uint32_t (*cnt)[16], PrepRank& r) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    r.b[k] = __ballot(set[k]);
    if (lane == 0) (*cnt)[k * 4 + wave] = (uint32_t)__popcll(r.b[k]);
  }
  __syncthreads();
  uint32_t p = 0, e = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    for (; e < (uint32_t)k * 4u + wave; e++) p += (*cnt)[e];
    r.before[k] = p;
  }
}

// ---- frustum selection -------------------------------------------------------------------------------------------
struct FrustumArgs {
  const float* xyz; const int32_t* rows; const float* proj;
  const float* scaling; const float* rotation; const float* opacity;
  float lo, hi;                      // -1 - padding, 1 + padding, narrowed to fp32 as torch narrows the Python scalars
  uint32_t n; int32_t num_points;
  uint8_t* flag; int64_t* pos; int64_t* row_out;
  float* o_xyz; float* o_scaling; float* o_rotation; float* o_opacity;
  uint32_t* chunk; uint32_t* total;
};

LR_DEV int32_t frustum_row(const FrustumArgs& a, uint32_t i) {
  const int32_t r = a.rows ? a.rows[i] : (int32_t)i;
  return (r >= 0 && r < a.num_points) ? r : -1;
}

// level_of_gaussian.py:44-52: h = [x, y, z, 1] @ M (the dot products as lr_radius_one forms them), pw = 1 / (hw + 1e-7),
// p = h * pw, six strict comparisons: a NaN or an infinity anywhere fails at least one of them
LR_DEV bool frustum_test(const FrustumArgs& a, int32_t r) {
  const float x = a.xyz[3 * (size_t)r], y = a.xyz[3 * (size_t)r + 1], z = a.xyz[3 * (size_t)r + 2];
  const float* __restrict__ m = a.proj;
  const float hx = lr_dot3p(m[0], m[4], m[8], x, y, z, m[12]);
  const float hy = lr_dot3p(m[1], m[5], m[9], x, y, z, m[13]);
  const float hz = lr_dot3p(m[2], m[6], m[10], x, y, z, m[14]);
  const float hw = lr_dot3p(m[3], m[7], m[11], x, y, z, m[15]);
  const float pw = 1.0f / (hw + 0.0000001f);
  const float px = hx * pw, py = hy * pw, depth = hz * pw;
  return depth > 0.f && depth < 1.f && px > a.lo && px < a.hi && py > a.lo && py < a.hi;
}

__global__ void __launch_bounds__(256)
frustum_flag_kernel(FrustumArgs a) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.x;
  uint32_t nk = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t i = chunk * PREP_CHUNK + (uint32_t)k * 256u + threadIdx.x;
    bool keep = false;
    if (i < a.n) {
      const int32_t r = frustum_row(a, i);
      keep = r >= 0 && frustum_test(a, r);
      a.flag[i] = keep ? 1 : 0;
    }
    nk += (uint32_t)__popcll(__ballot(keep));
  }
  if (lane == 0) wsum[wave] = nk;
  __syncthreads();
  if (threadIdx.x == 0) a.chunk[chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive prefixes of `count` per-chunk counts in place, their sum to *total.  The number of entries is n_host, or
// *n_dev (capped at cap) when the size lives on the device.
__global__ void __launch_bounds__(1024)
prep_scan_kernel(uint32_t* __restrict__ chunk, uint32_t n_host, const uint32_t* __restrict__ n_dev, uint32_t cap,
                 uint32_t* __restrict__ total) {
  __shared__ uint32_t ws[16];
  const uint32_t n = n_dev ? min(*n_dev, cap) : n_host;
  const uint32_t nchunks = (n + PREP_CHUNK - 1) / PREP_CHUNK;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t run = 0;
  for (uint32_t base = 0; base < nchunks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nchunks ? chunk[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(inc, d);
      if ((int)lane >= d) inc += u;
    }
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16u; w++) {
      const uint32_t t = ws[w];
      if (w < wave) off += t;
      tot += t;
    }
    if (i < nchunks) chunk[i] = run + off + inc - v;
    run += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = run;
}

// The activations are those of the gather kernel (sh.hip: ga_fwd_kernel), expression for expression, so the root render
// sees the bits LoG.get_all would hand the rasterizer for the same rows.
__global__ void __launch_bounds__(256)
frustum_scatter_kernel(FrustumArgs a) {
  __shared__ uint32_t cnt[16];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t chunk = blockIdx.x;
  bool set[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t i = chunk * PREP_CHUNK + (uint32_t)k * 256u + threadIdx.x;
    set[k] = i < a.n && a.flag[i] != 0;
  }
  PrepRank rk;
  prep_rank(set, &cnt, rk);
  const uint32_t base = a.chunk[chunk];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (!set[k]) continue;
    const uint32_t i = chunk * PREP_CHUNK + (uint32_t)k * 256u + threadIdx.x;
    const size_t d = (size_t)base + rk.before[k] + (uint32_t)__popcll(rk.b[k] & below);   // < n: a rank among n entries
    const int32_t r = frustum_row(a, i);                                                  // >= 0: the flag is set
    a.pos[d] = (int64_t)i;
    if (a.row_out) a.row_out[d] = (int64_t)r;
    if (a.o_xyz) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        a.o_xyz[3 * d + c] = a.xyz[3 * (size_t)r + c];
        a.o_scaling[3 * d + c] = expf(a.scaling[3 * (size_t)r + c]);
      }
      const float4 q4 = reinterpret_cast<const float4*>(a.rotation)[r];
      const float q[4] = {q4.x, q4.y, q4.z, q4.w};
      const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
      a.o_rotation[4 * d] = q[0] / nrm; a.o_rotation[4 * d + 1] = q[1] / nrm;
      a.o_rotation[4 * d + 2] = q[2] / nrm; a.o_rotation[4 * d + 3] = q[3] / nrm;
      a.o_opacity[d] = ga_sigmoid(a.opacity[r]);
    }
  }
}

static inline size_t prep_chunks(size_t n) { return n / PREP_CHUNK + 1; }
static inline size_t prep_align4(size_t w) { return (w + 3) & ~(size_t)3; }

size_t lr_frustum_scratch_bytes(int n) { return 4 * (4 + prep_align4(prep_chunks((size_t)(n > 0 ? n : 0)))); }

hipError_t lr_launch_frustum(int n, int num_points, const float* xyz, const int32_t* rows, const float* proj, float lo,
                             float hi, const float* scaling, const float* rotation, const float* opacity, uint8_t* flag,
                             int64_t* pos, int64_t* row_out, float* o_xyz, float* o_scaling, float* o_rotation,
                             float* o_opacity, void* scratch, hipStream_t s) {
  uint32_t* w = reinterpret_cast<uint32_t*>(scratch);
  FrustumArgs a;
  a.xyz = xyz; a.rows = rows; a.proj = proj; a.scaling = scaling; a.rotation = rotation; a.opacity = opacity;
  a.lo = lo; a.hi = hi; a.n = (uint32_t)n; a.num_points = num_points;
  a.flag = flag; a.pos = pos; a.row_out = row_out;
  a.o_xyz = o_xyz; a.o_scaling = o_scaling; a.o_rotation = o_rotation; a.o_opacity = o_opacity;
  a.total = w; a.chunk = w + 4;
  const uint32_t chunks = ((uint32_t)n + PREP_CHUNK - 1) / PREP_CHUNK;
  if (chunks) hipLaunchKernelGGL(frustum_flag_kernel, dim3(chunks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(prep_scan_kernel, dim3(1), dim3(1024), 0, s, a.chunk, (uint32_t)n, (const uint32_t*)nullptr, 0u, a.total);
  if (chunks) hipLaunchKernelGGL(frustum_scatter_kernel, dim3(chunks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- root filter: level_of_gaussian.py:241-242 -------------------------------------------------------------------
// Root k of the in-range roots stays when point_weight[k] > 1e-8; a dropped root becomes -1 in the traversal's root
// list (lod.hip skips it, order kept) and its entry of root_flag is cleared.
__global__ void __launch_bounds__(256)
prep_root_filter_kernel(uint32_t k_roots, const int64_t* __restrict__ rows, const float* __restrict__ weight,
                        const int64_t* __restrict__ pos, uint8_t* __restrict__ root_flag, uint32_t num_flags,
                        int64_t* __restrict__ rows_out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= k_roots) return;
  const bool keep = weight[k] > 1e-8f;
  rows_out[k] = keep ? rows[k] : (int64_t)-1;
  const int64_t p = pos[k];
  if (!keep && p >= 0 && p < (int64_t)num_flags) root_flag[p] = 0;
}

hipError_t lr_launch_root_filter(int k_roots, const int64_t* rows, const float* weight, const int64_t* pos,
                                 uint8_t* root_flag, int num_flags, int64_t* rows_out, hipStream_t s) {
  if (k_roots > 0)
    hipLaunchKernelGGL(prep_root_filter_kernel, dim3(((uint32_t)k_roots + 255u) / 256u), dim3(256), 0, s, (uint32_t)k_roots,
                       rows, weight, pos, root_flag, (uint32_t)num_flags, rows_out);
  return hipGetLastError();
}

// ---- leaf / node partition: level_of_gaussian.py:244-251 ---------------------------------------------------------
struct PartArgs {
  const int64_t* list; const uint32_t* n_dev; uint32_t cap;
  const int32_t* node_index; const int8_t* depth;
  int32_t num_points, all_levels, current_depth;
  int64_t* out_leaf; int64_t* out_node;
  uint32_t* chunk; uint32_t* leaf_total;
};

LR_DEV bool part_is_leaf(const PartArgs& a, int64_t r) {
  if (r < 0 || r >= (int64_t)a.num_points) return false;
  const int32_t d = (int32_t)a.depth[r];
  return a.all_levels ? (a.node_index[r] == -1 && d > 0) : (d == a.current_depth);
}

template <bool SCATTER>
__global__ void __launch_bounds__(256)
prep_part_kernel(PartArgs a) {
  __shared__ uint32_t cnt[16];
  const uint32_t n = min(*a.n_dev, a.cap);
  const uint32_t nchunks = (n + PREP_CHUNK - 1) / PREP_CHUNK;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    int64_t r[4];
    bool leaf[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * PREP_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      r[k] = i < n ? a.list[i] : (int64_t)-1;
      leaf[k] = i < n && part_is_leaf(a, r[k]);
    }
    PrepRank rk;
    prep_rank(leaf, &cnt, rk);
    if (!SCATTER) {
      if (threadIdx.x == 255) a.chunk[chunk] = rk.before[3] + (uint32_t)__popcll(rk.b[3]);   // (k, wave) = (3, 3): the last
    } else {
      const uint32_t base = a.chunk[chunk];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t i = chunk * PREP_CHUNK + (uint32_t)k * 256u + threadIdx.x;
        if (i >= n) continue;
        const uint32_t leaves_before = base + rk.before[k] + (uint32_t)__popcll(rk.b[k] & below);
        if (leaf[k]) a.out_leaf[leaves_before] = r[k];      // < n <= cap
        else a.out_node[i - leaves_before] = r[k];          // <= i < cap
      }
    }
    __syncthreads();
  }
}

size_t lr_partition_scratch_bytes(uint32_t capacity) { return 4 * prep_align4(prep_chunks(capacity)); }

hipError_t lr_launch_partition(const int64_t* list, const uint32_t* n_dev, uint32_t capacity, const int32_t* node_index,
                               const int8_t* depth, int num_points, int all_levels, int current_depth, int64_t* out_leaf,
                               int64_t* out_node, uint32_t* chunk, uint32_t* leaf_total, hipStream_t s) {
  PartArgs a;
  a.list = list; a.n_dev = n_dev; a.cap = capacity; a.node_index = node_index; a.depth = depth;
  a.num_points = num_points; a.all_levels = all_levels; a.current_depth = current_depth;
  a.out_leaf = out_leaf; a.out_node = out_node; a.chunk = chunk; a.leaf_total = leaf_total;
  const size_t chunks = ((size_t)capacity + PREP_CHUNK - 1) / PREP_CHUNK;
  const uint32_t grid = (uint32_t)(chunks < 1 ? 1 : (chunks > 2048 ? 2048 : chunks));
  hipLaunchKernelGGL(prep_part_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(prep_scan_kernel, dim3(1), dim3(1024), 0, s, chunk, 0u, n_dev, capacity, leaf_total);
  hipLaunchKernelGGL(prep_part_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- LoG.clamp_scale ---------------------------------------------------------------------------------------------
// torch.clamp(x, lo, hi) with tensor bounds: a NaN in x, lo or hi (in that order) is the result, otherwise
// min(max(x, lo), hi) -- so lo > hi gives hi.
LR_DEV float prep_clamp(float x, float lo, float hi) {
  if (x != x) return x;
  if (lo != lo) return lo;
  if (hi != hi) return hi;
  return fminf(fmaxf(x, lo), hi);
}

__global__ void __launch_bounds__(256)
prep_clamp_kernel(uint32_t m, const int64_t* __restrict__ index, const uint8_t* __restrict__ flag, int32_t num_points,
                  float* __restrict__ scaling, const float* __restrict__ rmin, const float* __restrict__ rmax) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  if (flag && !flag[i]) return;
  const int64_t r = index[i];
  if (r < 0 || r >= (int64_t)num_points) return;
  const float lo = logf(rmin[r]), hi = logf(rmax[r]);
#pragma unroll
  for (int c = 0; c < 3; c++) scaling[3 * (size_t)r + c] = prep_clamp(scaling[3 * (size_t)r + c], lo, hi);
}

hipError_t lr_launch_clamp_scale(int m, const int64_t* index, const uint8_t* flag, int num_points, float* scaling,
                                 const float* rmin, const float* rmax, hipStream_t s) {
  if (m > 0)
    hipLaunchKernelGGL(prep_clamp_kernel, dim3(((uint32_t)m + 255u) / 256u), dim3(256), 0, s, (uint32_t)m, index, flag,
                       num_points, scaling, rmin, rmax);
  return hipGetLastError();
}
