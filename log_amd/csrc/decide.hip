// decide.hip -- the decision layer of LoG's densification (/root/reference/LoG/model/level_of_gaussian.py):
//   * LoG.update_depth_stage :454-508 up to the flags it hands to TensorTree.split_and_remove: one pass over the rows gives
//     flag_split / flag_remove, the counts of its log lines, the depth histograms and the four str_min_mean_max lines; the
//     top-k cut (:492-499) is a radix select on the candidates' radii_max_max -- four 8-bit digits, histograms privatised in
//     LDS and flushed with integer atomics, one workgroup picks the digit -- and a last pass that drops the rows under the
//     threshold.  The select and the drop return at once when the pass before found that no cut is needed;
//   * LoG.update_init_stage :400-427 ('split_by_2d'): one pass, the same kind of record;
//   * :516-519, radius3d_max of the new children from their parents' scaling, after the resize.
// Statistics: every workgroup leaves one partial per line (count, min, max, sum and sum of squares in double, waves and
// lanes combined in a fixed order), one workgroup combines the partials in index order.  No floating-point atomic: the grid
// depends on p alone, so two runs give the same bits.
#include "decide.hpp"

#define DEC_CHUNK 1024u
#define DEC_MAX_PARTS 2048u

struct DecWork {
  uint32_t digit[256];     // the digit histogram of the running select pass
  uint32_t active;         // a cut is needed and num_max_split > 0
  uint32_t k_rem;          // rank still to find among the rows whose higher digits equal prefix
  uint32_t prefix;         // the digits found so far (of value ^ 0x80000000: unsigned order = signed order)
  uint32_t pad;
};
struct DecScratch {
  lograst_decide_record rec;
  DecWork work;
  lograst_decide_stat part[DEC_MAX_PARTS][4];
};

struct DecAcc { double sum, sumsq; float mn, mx; uint32_t n; };

// torch.min / torch.max: a NaN anywhere is the result
LR_DEV float dec_min(float a, float x) { return (a != a) ? a : ((x < a || x != x) ? x : a); }
LR_DEV float dec_max(float a, float x) { return (a != a) ? a : ((x > a || x != x) ? x : a); }
LR_DEV void dec_clear(DecAcc& s) { s.sum = 0.0; s.sumsq = 0.0; s.mn = INFINITY; s.mx = -INFINITY; s.n = 0u; }
LR_DEV void dec_add(DecAcc& s, float x, uint32_t w = 1u) {
  const double d = (double)x, dw = (double)w;
  s.sum += dw * d; s.sumsq += dw * (d * d);
  s.mn = dec_min(s.mn, x); s.mx = dec_max(s.mx, x); s.n += w;
}
LR_DEV void dec_merge(DecAcc& s, const DecAcc& o) {
  s.sum += o.sum; s.sumsq += o.sumsq; s.mn = dec_min(s.mn, o.mn); s.mx = dec_max(s.mx, o.mx); s.n += o.n;
}

// the sum of a 256-thread workgroup's accumulators: xor butterfly inside each wave (both lanes of a pair add the same two
// numbers, so every lane ends with the same bits), then waves 0..3 in order.  Valid in thread 0.
LR_DEV DecAcc dec_block_sum(DecAcc s, DecAcc (*sh)[4]) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    DecAcc o;
    o.sum = __shfl_xor(s.sum, d); o.sumsq = __shfl_xor(s.sumsq, d);
    o.mn = __shfl_xor(s.mn, d); o.mx = __shfl_xor(s.mx, d); o.n = __shfl_xor(s.n, d);
    dec_merge(s, o);
  }
  __syncthreads();                                   // the previous use of sh is over
  if ((threadIdx.x & 63u) == 0) (*sh)[threadIdx.x >> 6] = s;
  __syncthreads();
  DecAcc t = (*sh)[0];
  dec_merge(t, (*sh)[1]); dec_merge(t, (*sh)[2]); dec_merge(t, (*sh)[3]);
  return t;
}

LR_DEV void dec_store(lograst_decide_stat& out, const DecAcc& s) {
  out.sum = s.sum; out.sumsq = s.sumsq; out.min = s.mn; out.max = s.mx; out.count = s.n; out.reserved = 0u;
}

LR_DEV uint32_t dec_count(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }

// wave-uniform counts -> LDS -> the record (integer atomics: any order gives the same sums)
LR_DEV void dec_flush_counts(const uint32_t* c, int n, uint32_t* s_cnt, uint32_t* out) {
  if ((threadIdx.x & 63u) == 0)
    for (int j = 0; j < n; j++) if (c[j]) atomicAdd(&s_cnt[j], c[j]);
  __syncthreads();
  if ((int)threadIdx.x < n && s_cnt[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_cnt[threadIdx.x]);
}

LR_DEV void dec_flush_hist(const uint32_t* s_hist, uint32_t* out) {   // 256 bins, 256 threads, after a __syncthreads()
  const uint32_t v = s_hist[threadIdx.x];
  if (v) atomicAdd(&out[threadIdx.x], v);
}

// ---- the depth stage ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
decide_depth_kernel(uint32_t p, lograst_decide_depth_args a, DecScratch* __restrict__ sc) {
  __shared__ uint32_t s_hist[3][256];
  __shared__ uint32_t s_cnt[8];
  __shared__ DecAcc s_acc[4];
  for (int h = 0; h < 3; h++) s_hist[h][threadIdx.x] = 0u;
  if (threadIdx.x < 8u) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  DecAcc st[4];
#pragma unroll
  for (int j = 0; j < 4; j++) dec_clear(st[j]);
  uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
  const uint32_t nchunks = (p + DEC_CHUNK - 1) / DEC_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DEC_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      const bool in = i < p;
      bool sg = false, sr = false, cand = false, rem = false, lt = false, parent = false;
      int32_t d = 0;
      float grad = 0.f, rmm_f = 0.f;
      if (in) {
        d = (int32_t)a.depth[i];
        const bool leaf = a.node_index[i] == -1;
        const int32_t area = a.area_sum[i];
        grad = a.grad_sum[i] / (float)(area > 1 ? area : 1);
        rmm_f = (float)a.radii_max_max[i];
        lt = d < a.current_depth;
        parent = leaf && lt;
        sg = grad > a.split_grad_thres;
        sr = rmm_f > a.radius2d_thres;
        rem = leaf && d > 0 && a.weights_max[i] < a.remove_weights_thres && (int32_t)a.visible_count[i] > 1;
        cand = sg && sr && parent && a.create_steps[i] > a.min_steps_split && !rem;
        a.flag_split[i] = cand ? 1 : 0;
        a.flag_remove[i] = rem ? 1 : 0;
      }
      c[LOGRAST_DECIDE_SPLIT_GRAD] += dec_count(sg);
      c[LOGRAST_DECIDE_SPLIT_RADII] += dec_count(sr);
      c[LOGRAST_DECIDE_CANDIDATES] += dec_count(cand);
      c[LOGRAST_DECIDE_REMOVED] += dec_count(rem);
      c[LOGRAST_DECIDE_DEPTH_LT] += dec_count(lt);
      // the depth histogram: a wave whose rows share one depth (the usual case) adds its count once
      const uint32_t bin = (uint32_t)(d + 128);
      const uint64_t live = __ballot(in);
      if (live) {
        const uint32_t first = __shfl(bin, (int)__ffsll((long long)live) - 1);
        if (__ballot(in && bin == first) == live) {
          if ((threadIdx.x & 63u) == 0) atomicAdd(&s_hist[0][first], (uint32_t)__popcll(live));
        } else if (in) {
          atomicAdd(&s_hist[0][bin], 1u);
        }
      }
      if (cand && d < a.max_level) atomicAdd(&s_hist[1][bin], 1u);
      if (rem) atomicAdd(&s_hist[2][bin], 1u);
      if (parent) {
        dec_add(st[0], ga_sigmoid(a.opacity[i]));
        const float e0 = expf(a.scaling[3 * (size_t)i]), e1 = expf(a.scaling[3 * (size_t)i + 1]),
                    e2 = expf(a.scaling[3 * (size_t)i + 2]);
        const float mx = fmaxf(fmaxf(e0, e1), e2), mn = fminf(fminf(e0, e1), e2);
        const float mid = ((e0 + e1) + e2) - mx - mn;
        dec_add(st[1], mx / mid);
        dec_add(st[2], grad);
        dec_add(st[3], rmm_f);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const DecAcc t = dec_block_sum(st[j], &s_acc);
    if (threadIdx.x == 0) dec_store(sc->part[blockIdx.x][j], t);
  }
  dec_flush_counts(c, 5, s_cnt, sc->rec.counts);
  dec_flush_hist(s_hist[0], sc->rec.depth_all);
  dec_flush_hist(s_hist[1], sc->rec.depth_split);
  dec_flush_hist(s_hist[2], sc->rec.depth_remove);
}

// One workgroup: the partials of `nparts` workgroups in index order, then (depth stage) whether a cut is needed.
__global__ void __launch_bounds__(256)
decide_finish_kernel(DecScratch* __restrict__ sc, uint32_t nparts, int depth_stage, int32_t max_split_points) {
  __shared__ DecAcc s_acc[4];
  for (int j = 0; j < 4; j++) {
    DecAcc s;
    dec_clear(s);
    for (uint32_t i = threadIdx.x; i < nparts; i += 256u) {
      const lograst_decide_stat& q = sc->part[i][j];
      DecAcc o;
      o.sum = q.sum; o.sumsq = q.sumsq; o.mn = q.min; o.mx = q.max; o.n = q.count;
      dec_merge(s, o);
    }
    const DecAcc t = dec_block_sum(s, &s_acc);
    if (threadIdx.x == 0) dec_store(sc->rec.stats[j], t);
  }
  if (threadIdx.x == 0 && depth_stage) {
    // level_of_gaussian.py:492: min(int(depth_minus1_sum * 0.05), max_split_points) -- an integer tensor times a Python
    // float is torch's fp32 product, int() truncates
    const float f = (float)sc->rec.counts[LOGRAST_DECIDE_DEPTH_LT] * 0.05f;
    int32_t k = (int32_t)f;
    if (k > max_split_points) k = max_split_points;
    const bool need = k >= 0 && sc->rec.counts[LOGRAST_DECIDE_CANDIDATES] > (uint32_t)k;
    sc->rec.num_max_split = (uint32_t)(k > 0 ? k : 0);
    sc->rec.need_cut = (need || k < 0) ? 1u : 0u;      // a negative cap: the reference's topk raises, as with k == 0
    sc->work.active = (need && k > 0) ? 1u : 0u;
    sc->work.k_rem = (uint32_t)(k > 0 ? k : 0);
    sc->work.prefix = 0u;
  }
}

LR_DEV uint32_t dec_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

// digit SHIFT / 8 of the candidates whose higher digits equal the prefix found so far
template <int SHIFT>
__global__ void __launch_bounds__(256)
decide_digit_kernel(uint32_t p, const uint8_t* __restrict__ flag_split, const int32_t* __restrict__ radii,
                    DecScratch* __restrict__ sc) {
  if (!sc->work.active) return;
  __shared__ uint32_t s_hist[256];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t prefix = sc->work.prefix;
  const uint32_t nchunks = (p + DEC_CHUNK - 1) / DEC_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DEC_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      if (i < p && flag_split[i]) {
        const uint32_t key = dec_key(radii[i]);
        if (SHIFT == 24 || ((key ^ prefix) >> (SHIFT + 8)) == 0u) atomicAdd(&s_hist[(key >> SHIFT) & 255u], 1u);
      }
    }
  }
  __syncthreads();
  dec_flush_hist(s_hist, sc->work.digit);
}

// One workgroup: the largest digit d with  #(digit > d) < k_rem <= #(digit >= d);  the histogram is cleared for the next pass.
template <int SHIFT>
__global__ void __launch_bounds__(256)
decide_pick_kernel(DecScratch* __restrict__ sc) {
  if (!sc->work.active) return;
  __shared__ uint32_t s_hist[256];
  s_hist[threadIdx.x] = sc->work.digit[threadIdx.x];
  sc->work.digit[threadIdx.x] = 0u;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t k = sc->work.k_rem;      // 1 <= k <= the number of candidates counted in s_hist
  uint32_t above = 0u, d = 0u;
  for (int b = 255; b >= 0; b--) {
    if (above + s_hist[b] >= k) { d = (uint32_t)b; break; }
    above += s_hist[b];
  }
  const uint32_t prefix = sc->work.prefix | (d << SHIFT);
  sc->work.prefix = prefix;
  sc->work.k_rem = k - above;
  if (SHIFT == 0) {
    const int32_t v = (int32_t)(prefix ^ 0x80000000u);
    sc->rec.cut_value = v;
    sc->rec.cut_thres = (float)v;
  }
}

// :499  flag_split & (radii_max_max.float() >= new_radii_thres): the rows under the threshold leave flag_split
__global__ void __launch_bounds__(256)
decide_cut_kernel(uint32_t p, uint8_t* __restrict__ flag_split, const int32_t* __restrict__ radii,
                  const int8_t* __restrict__ depth, int32_t max_level, DecScratch* __restrict__ sc) {
  if (!sc->work.active) return;
  __shared__ uint32_t s_hist[256];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const float thres = sc->rec.cut_thres;
  const uint32_t nchunks = (p + DEC_CHUNK - 1) / DEC_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DEC_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      if (i < p && flag_split[i] && !((float)radii[i] >= thres)) {
        flag_split[i] = 0;
        const int32_t d = (int32_t)depth[i];
        if (d < max_level) atomicAdd(&s_hist[(uint32_t)(d + 128)], 1u);
      }
    }
  }
  __syncthreads();
  const uint32_t v = s_hist[threadIdx.x];
  if (v) atomicSub(&sc->rec.depth_split[threadIdx.x], v);
}

// ---- the init stage ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
decide_init_kernel(uint32_t p, lograst_decide_init_args a, DecScratch* __restrict__ sc) {
  __shared__ uint32_t s_cnt[8];
  __shared__ DecAcc s_acc[4];
  if (threadIdx.x < 8u) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  DecAcc st[4];
#pragma unroll
  for (int j = 0; j < 4; j++) dec_clear(st[j]);
  uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
  const uint32_t nchunks = (p + DEC_CHUNK - 1) / DEC_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DEC_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      const bool in = i < p;
      bool rw = false, nonmax = false, small = false, by_grad = false, by_radii = false;
      if (in) {
        const float wmax = a.weights_max[i];
        const int32_t rmm = a.radii_max_max[i];
        const float rmm_f = (float)rmm;
        const int32_t area = a.area_sum[i];
        const float grad = a.grad_sum[i] / (float)(area > 1 ? area : 1);
        rw = wmax < a.init_weight_min;
        nonmax = wmax < ga_sigmoid(a.opacity[i]) * 0.1f;
        small = rmm_f < a.small_thres;
        const bool rem = (small && a.rand[i] > 0.5f) || rw || nonmax;
        const bool act = a.create_steps[i] > a.min_steps && rmm_f > 0.f;
        by_grad = grad > a.grad_thres && rmm_f > a.radius_thres;
        by_radii = rmm_f > a.split_thres_sq;
        const bool split = act && (by_radii || by_grad) && !rem;
        a.flag_split[i] = split ? 1 : 0;
        a.flag_remove[i] = rem ? 1 : 0;
        if (act) dec_add(st[0], rmm_f);
        dec_add(st[1], grad);
        if (split) dec_add(st[2], rmm_f);
        if (split || !rem) dec_add(st[3], a.radius3d_min[i], split ? (uint32_t)a.children : 1u);
      }
      c[LOGRAST_DECIDE_REMOVE_WEIGHT] += dec_count(rw);
      c[LOGRAST_DECIDE_NONMAX] += dec_count(nonmax);
      c[LOGRAST_DECIDE_REMOVE_SMALL] += dec_count(small);
      c[LOGRAST_DECIDE_INIT_SPLIT_GRAD] += dec_count(by_grad);
      c[LOGRAST_DECIDE_INIT_SPLIT_RADII] += dec_count(by_radii);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const DecAcc t = dec_block_sum(st[j], &s_acc);
    if (threadIdx.x == 0) dec_store(sc->part[blockIdx.x][j], t);
  }
  dec_flush_counts(c, 5, s_cnt, sc->rec.counts);
}

// ---- :516-519 after the resize -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
decide_child_radius_kernel(uint32_t num_points, uint32_t num_children, const int32_t* __restrict__ index_parent,
                           const float* __restrict__ scaling, float decay, float* __restrict__ radius3d_max) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= num_children) return;
  const uint32_t j = num_points - num_children + t;
  const int32_t par = index_parent[j];
  if (par < 0 || (uint32_t)par >= num_points) return;
  const float e0 = expf(scaling[3 * (size_t)par]), e1 = expf(scaling[3 * (size_t)par + 1]),
              e2 = expf(scaling[3 * (size_t)par + 2]);
  radius3d_max[j] = decay * fmaxf(fmaxf(e0, e1), e2);
}

// ---- launches ----------------------------------------------------------------------------------------------------
size_t lr_decide_scratch_bytes(int) { return sizeof(DecScratch); }

static inline uint32_t dec_grid(uint32_t p) {
  const uint32_t chunks = (p + DEC_CHUNK - 1) / DEC_CHUNK;
  return chunks < DEC_MAX_PARTS ? chunks : DEC_MAX_PARTS;
}

hipError_t lr_launch_decide_depth(int p, const lograst_decide_depth_args& a, void* scratch, hipStream_t s) {
  DecScratch* sc = reinterpret_cast<DecScratch*>(scratch);
  hipError_t e = hipMemsetAsync(scratch, 0, offsetof(DecScratch, part), s);
  if (e != hipSuccess) return e;
  const uint32_t n = (uint32_t)p, grid = dec_grid(n);
  if (grid) hipLaunchKernelGGL(decide_depth_kernel, dim3(grid), dim3(256), 0, s, n, a, sc);
  hipLaunchKernelGGL(decide_finish_kernel, dim3(1), dim3(256), 0, s, sc, grid, 1, a.max_split_points);
  if (!grid) return hipGetLastError();
  hipLaunchKernelGGL(decide_digit_kernel<24>, dim3(grid), dim3(256), 0, s, n, a.flag_split, a.radii_max_max, sc);
  hipLaunchKernelGGL(decide_pick_kernel<24>, dim3(1), dim3(256), 0, s, sc);
  hipLaunchKernelGGL(decide_digit_kernel<16>, dim3(grid), dim3(256), 0, s, n, a.flag_split, a.radii_max_max, sc);
  hipLaunchKernelGGL(decide_pick_kernel<16>, dim3(1), dim3(256), 0, s, sc);
  hipLaunchKernelGGL(decide_digit_kernel<8>, dim3(grid), dim3(256), 0, s, n, a.flag_split, a.radii_max_max, sc);
  hipLaunchKernelGGL(decide_pick_kernel<8>, dim3(1), dim3(256), 0, s, sc);
  hipLaunchKernelGGL(decide_digit_kernel<0>, dim3(grid), dim3(256), 0, s, n, a.flag_split, a.radii_max_max, sc);
  hipLaunchKernelGGL(decide_pick_kernel<0>, dim3(1), dim3(256), 0, s, sc);
  hipLaunchKernelGGL(decide_cut_kernel, dim3(grid), dim3(256), 0, s, n, a.flag_split, a.radii_max_max, a.depth, a.max_level, sc);
  return hipGetLastError();
}

hipError_t lr_launch_decide_init(int p, const lograst_decide_init_args& a, void* scratch, hipStream_t s) {
  DecScratch* sc = reinterpret_cast<DecScratch*>(scratch);
  hipError_t e = hipMemsetAsync(scratch, 0, offsetof(DecScratch, part), s);
  if (e != hipSuccess) return e;
  const uint32_t n = (uint32_t)p, grid = dec_grid(n);
  if (grid) hipLaunchKernelGGL(decide_init_kernel, dim3(grid), dim3(256), 0, s, n, a, sc);
  hipLaunchKernelGGL(decide_finish_kernel, dim3(1), dim3(256), 0, s, sc, grid, 0, 0);
  return hipGetLastError();
}

hipError_t lr_launch_child_radius_max(int num_points, int num_children, const int32_t* index_parent, const float* scaling,
                                      float scaling_decay, float* radius3d_max, hipStream_t s) {
  if (num_children > 0)
    hipLaunchKernelGGL(decide_child_radius_kernel, dim3(((uint32_t)num_children + 255u) / 256u), dim3(256), 0, s,
                       (uint32_t)num_points, (uint32_t)num_children, index_parent, scaling, scaling_decay, radius3d_max);
  return hipGetLastError();
}
