// accumulate.hip -- steps over several views of the LoG model: every view's activation backward is ADDED into sums laid out
// by model row, and one Adam step is taken over the rows some view saw.
// The arithmetic is not written here: the chain rule, the SH row fill, the map of a row's 14 small values and the halves of
// the Adam update live in sh_basis.hpp (the element update itself, lr_adam_elem, in common.hpp), one definition each, called
// by these kernels and by those of sh.hip and counter.hip.  This file holds the two kernels' memory access.
//   * lr_launch_activate_bwd_accumulate : ga_bwd_kernel's gradients (sh.hip; the same functions, dL/dxyz passed through) of the
//                                         rows with radii > 0, added into row index[r] of six strided targets; seen[index[r]]
//                                         += 1.  Plain read-modify-writes: a view's index has no duplicates and the views follow
//                                         each other on the stream, so the sums are taken in view order and the same views
//                                         give the same bits.
//   * lr_launch_accumulated_adam        : adam_kernel's update (counter.hip; the same function) of every row with seen > 0, from
//                                         the accumulated gradient, which is zero-filled on the way, as seen is: what the step
//                                         clears is what the views touched, not P x (14 + 3 K) floats.
// Both are streaming kernels with a scattered (first) or a masked (second) row access: HBM-bound.
// Derived traffic per live row, K coefficients: the first kernel reads 14 upstream + 11 raw floats (colours' upstream 3,
// scaling 3 + 3, opacity 1 + 1, rotation 4 + 4, xyz 3 + 3 of which the raw xyz only when a degree is active) = up to 100
// bytes, its index and radii (12 bytes), and reads and writes (14 + 3 K) floats of sums and one count:
// 112 + 8 (14 + 3 K) + 8 bytes = 592 at K = 15.  The second reads 4 bytes per MODEL row and writes 1, and per seen row
// reads gradient, parameter and two (amsgrad: three) moments and writes all of them back: 32 (40) bytes per element,
// 1888 (2360) at K = 15.
#include "common.hpp"
#include "launch.hpp"

static __constant__ float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                    -1.0925484305920792f, 0.5462742152960396f};
static __constant__ float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                    -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
#define LR_SH_TABLES_DEFINED
#include "sh_basis.hpp"   // lr_sh_basis (reads the two tables above) and everything the row kernels of both files share

// ---- one view's activation backward, added by model row ---------------------------------------------------------------
// One lane per compact row, as ga_bwd_kernel: the 14 small values (ga_act_grads) stay in the lane (all old sums requested,
// then all stores); the 3 K SH gradients (ga_sh_grad_row) go through the wave's LDS rows so that the wave walks them
// contiguously.  What is this kernel's own is where the values go: read-modify-writes of the strided targets.
// key order: 0 xyz, 1 scaling, 2 opacity, 3 rotation, 4 colors, 5 shs (base == nullptr: not accumulated).
__global__ void __launch_bounds__(256)
acc_bwd_kernel(ActBwdArgs a, AccArgs t) {
  extern __shared__ float lr_sh_lds[];
  __shared__ long long lr_rowidx[4][64];
  const int L = 3 * a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);
  if (i0 >= a.n) return;
  const int rows = min(64, a.n - i0);
  const int i = i0 + lane;
  const bool ok = i < a.n;
  long long row = -1;                                       // the model row this lane adds into (-1: not visible / no row)
  if (ok && t.radii[i] > 0) {
    row = t.index[i];
    if (row < 0 || row >= (long long)t.num_points) row = -1;
  }
  float gc[3] = {0.f, 0.f, 0.f};
  if (row >= 0) {
    const size_t c = (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; k++) gc[k] = a.g_a_colors[3 * c + k];
    // the row's 14 small values; a key without a target is not loaded
    unsigned want = 0;
#pragma unroll
    for (int key = 0; key < 5; key++) want |= t.t[key].base ? GA_KEY(key) : 0u;
    float g[14], old[14];
    float* p[14];
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = (want & GA_KEY(0)) ? t.g_a_xyz[3 * c + k] : 0.f;
    ga_act_grads(a, c, want, gc, g);
#pragma unroll
    for (int k = 0; k < 14; k++) {
      const AccTarget& tk = t.t[ga_small(k).key];
      p[k] = tk.base ? tk.base + lr_acc_offset(row, tk.stride, ga_small(k).col) : nullptr;
    }
    // all old sums requested, then all stores
#pragma unroll
    for (int k = 0; k < 14; k++) old[k] = p[k] ? *p[k] : 0.f;
    const int32_t cnt = t.seen[row];
#pragma unroll
    for (int k = 0; k < 14; k++)
      if (p[k]) *p[k] = old[k] + g[k];
    t.seen[row] = cnt + 1;
  }
  if (L > 0 && t.t[5].base) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    lr_rowidx[wave][lane] = row;
    if (row >= 0) ga_sh_grad_row(a, i, gc, wl + lane * (L + 1));
    lr_sh_wave_sync();
    // the wave walks its rows' L gradients contiguously: element x = (row r, column c) of the wave's block; the model side
    // is one contiguous 4 L-byte piece per visible row.  GA_SH_UNROLL elements per lane in flight.
    const uint32_t magic = 0xffffffffu / (uint32_t)L + 1u;    // x / L for x < 65536 (L >= 3)
    const int total = rows * L;
    for (int x0 = lane; x0 < total; x0 += 64 * GA_SH_UNROLL) {
      float* p[GA_SH_UNROLL];
      float g[GA_SH_UNROLL], old[GA_SH_UNROLL];
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) {
        const int x = x0 + 64 * u;
        p[u] = nullptr; g[u] = 0.f;
        if (x < total) {
          const int r = (int)__umulhi((uint32_t)x, magic), c = x - r * L;
          const long long mr = lr_rowidx[wave][r];
          if (mr >= 0) { p[u] = t.t[5].base + lr_acc_offset(mr, t.t[5].stride, c); g[u] = wl[r * (L + 1) + c]; }
        }
      }
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) old[u] = p[u] ? *p[u] : 0.f;
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++)
        if (p[u]) *p[u] = old[u] + g[u];
    }
  }
}

hipError_t lr_launch_activate_bwd_accumulate(const ActBwdArgs& a, const AccArgs& t, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  lr_ga_lds_once<acc_bwd_kernel>();
  lr_prof_begin(LRK_GATHER_BWD, s);
  hipLaunchKernelGGL(acc_bwd_kernel, dim3((a.n + 255) / 256), dim3(256), (a.K > 0 && t.t[5].base) ? lr_ga_lds_bytes(a.K) : 0, s,
                     a, t);
  lr_prof_end(LRK_GATHER_BWD, s);
  return hipGetLastError();
}

// ---- one Adam step over the rows some view saw --------------------------------------------------------------------------
// One lane per MODEL row: it reads the row's count, publishes moved = count > 0 and clears the count -- nobody else reads
// it: the wave's ballot carries the flags to the SH walk below.  A wave without a seen row ends there (5 bytes per row).
// A seen row's 14 small elements are updated by its lane, its 3 K SH elements by the wave, contiguously; every accumulated
// gradient is replaced by zero after it was read.
__global__ void __launch_bounds__(256)
acc_adam_kernel(AdamArgs f, AccStepArgs t) {
  const int lane = threadIdx.x & 63;
  const long long p0 = (long long)blockIdx.x * 256 + (threadIdx.x & ~63);
  if (p0 >= (long long)f.num_points) return;
  const long long p = p0 + lane;
  const bool ok = p < (long long)f.num_points;
  bool live = false;
  if (ok) {
    live = t.seen[p] > 0;
    if (t.moved) t.moved[p] = live ? 1 : 0;
    if (live) t.seen[p] = 0;
  }
  const uint64_t mask = __ballot(live);
  if (!mask) return;
  if (live) {
    // the row's 14 small values
    GaElem e[14];
    float* gp[14];
#pragma unroll
    for (int k = 0; k < 14; k++) {
      const int key = ga_small(k).key, col = ga_small(k).col;
      const AdamKey& key_k = f.key[key];
      e[k].on = key_k.model != nullptr;
      e[k].o = lr_acc_offset(p, key_k.width, col);
      gp[k] = e[k].on ? const_cast<float*>(key_k.grad) + lr_acc_offset(p, t.gstride[key], col) : nullptr;
      e[k].p0 = e[k].on ? key_k.model[e[k].o] : 0.f;
      e[k].g = e[k].on ? *gp[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 14; k++) ga_adam_load(f.key[ga_small(k).key], e[k]);
#pragma unroll
    for (int k = 0; k < 14; k++) {
      ga_adam_store(f.key[ga_small(k).key], f, e[k]);
      if (gp[k]) *gp[k] = 0.f;
    }
  }
  const AdamKey& sh = f.key[5];
  if (sh.model) {
    const int L = sh.width;
    const long long left = (long long)f.num_points - p0;
    const int rows = left < 64 ? (int)left : 64;
    const uint32_t magic = 0xffffffffu / (uint32_t)L + 1u;    // x / L for x < 65536 (L >= 3)
    const int total = rows * L;
    for (int x0 = lane; x0 < total; x0 += 64 * GA_SH_UNROLL) {
      GaElem e[GA_SH_UNROLL];
      float* gp[GA_SH_UNROLL];
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) {
        const int x = x0 + 64 * u;
        e[u].on = false; e[u].o = 0; e[u].p0 = 0.f; e[u].g = 0.f; gp[u] = nullptr;
        if (x < total) {
          const int r = (int)__umulhi((uint32_t)x, magic), c = x - r * L;
          if ((mask >> r) & 1ull) {
            e[u].on = true;
            e[u].o = lr_acc_offset(p0 + r, L, c);
            gp[u] = const_cast<float*>(sh.grad) + lr_acc_offset(p0 + r, t.gstride[5], c);
            e[u].p0 = sh.model[e[u].o];
            e[u].g = *gp[u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) ga_adam_load(sh, e[u]);
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) {
        ga_adam_store(sh, f, e[u]);
        if (gp[u]) *gp[u] = 0.f;
      }
    }
  }
}

hipError_t lr_launch_accumulated_adam(const AdamArgs& f, const AccStepArgs& t, hipStream_t s) {
  if (f.num_points <= 0) return hipSuccess;
  lr_prof_begin(LRK_ADAM, s);
  hipLaunchKernelGGL(acc_adam_kernel, dim3((uint32_t)(((long long)f.num_points + 255) / 256)), dim3(256), 0, s, f, t);
  lr_prof_end(LRK_ADAM, s);
  return hipGetLastError();
}
