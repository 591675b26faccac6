// sh.hip -- "next" row N2: the rasterizer packages' native `shs=` / `sh_degree` / `campos`
// inputs.  colour = max(0, 0.5 + sum_k basis_k(dir) * sh_k), dir = normalise(mean - campos), degrees 0..3,
// with the clamp mask cutting the gradient (published behaviour of the third-party kernel).  LoG itself never
// takes this path (it evaluates the same polynomial in PyTorch -- /root/reference/LoG/model/sh_utils.py:31-68,
// LoG/model/activation.py:27-34 -- and passes colors_precomp, LoG/render/renderer.py:144-145); the basis is
// pinned against that file in tests/test_sh.py.  Streaming, one thread per Gaussian, coefficients staged per wave.
#include "common.hpp"
#include "launch.hpp"

__constant__ float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                             -1.0925484305920792f, 0.5462742152960396f};
__constant__ float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                             -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
#define LR_SH_TABLES_DEFINED
#include "sh_basis.hpp"   // lr_sh_basis (reads the two tables above) and everything the row kernels of both files share

// Memory layout is [Gaussian][coefficient][channel] (L = 3*M floats per Gaussian): a lane walking its own
// coefficients reads 4 bytes out of every 192 (M = 16), one cache line per instruction per lane.  Instead every wave
// moves the 64*L contiguous floats of its 64 Gaussians with full-width coalesced accesses and transposes through
// LDS (row stride L+1 floats: odd, so the per-lane row walks are bank-conflict free).  Measured at 10 M Gaussians,
// degree 3: forward 2.68 -> 0.6 ms, backward 4.51 -> 1.25 ms (3.1 TB/s).

// wave-cooperative copy of `count` floats between global memory (contiguous) and the wave's LDS rows.  The float4 path
// needs whole float4s per row (L % 4 == 0) and a 16-byte aligned global address; `glob` is base + 64 * wave * L floats, so
// with L % 4 == 0 its alignment is the base pointer's: the test is wave-uniform.  Any other base (the C ABI asks for 4-byte
// alignment of shs / dl_dshs only) takes the scalar path, which gives the same bits.
template <bool TO_LDS, bool ADD = false>
LR_DEV void lr_sh_wave_copy(float* __restrict__ lds, float* __restrict__ glob, int L, int count, int lane) {
  const uint32_t magic = 0xffffffffu / (uint32_t)L + 1u;  // e / L for e < 65536
  if ((L & 3) == 0 && (reinterpret_cast<uintptr_t>(glob) & 15u) == 0) {
    for (int e = 4 * lane; e < count; e += 256) {  // count is a multiple of L, L of 4: float4s never straddle rows
      const int g = (int)__umulhi((uint32_t)e, magic), j = e - g * L;
      float* row = lds + g * (L + 1) + j;
      if (TO_LDS) {
        const float4 v = *reinterpret_cast<const float4*>(glob + e);
        row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
      } else {
        float4 o = float4{row[0], row[1], row[2], row[3]};
        if (ADD) {
          const float4 old = *reinterpret_cast<const float4*>(glob + e);
          o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
        } else {  // as the scalar path's `+ 0.f`: a gradient that came out as -0.0 (negative basis x cut channel) leaves as +0.0
          o.x += 0.f; o.y += 0.f; o.z += 0.f; o.w += 0.f;
        }
        *reinterpret_cast<float4*>(glob + e) = o;
      }
    }
  } else {
    for (int e = lane; e < count; e += 64) {
      const int g = (int)__umulhi((uint32_t)e, magic), j = e - g * L;
      if (TO_LDS) lds[g * (L + 1) + j] = glob[e];
      else glob[e] = lds[g * (L + 1) + j] + (ADD ? glob[e] : 0.f);
    }
  }
}

__global__ void __launch_bounds__(256)
lr_sh_fwd_kernel(int N, int deg, int M, const float* __restrict__ means, const float* __restrict__ campos,
                 const float* __restrict__ shs, float* __restrict__ colors, uint8_t* __restrict__ clamped) {
  extern __shared__ float lr_sh_lds[];  // 4 waves x 64 rows x (L+1)
  const int L = 3 * M, lane = threadIdx.x & 63;
  float* const wl = lr_sh_lds + (threadIdx.x >> 6) * 64 * (L + 1);
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);  // the wave's first Gaussian
  if (i0 >= N) return;
  const int rows = min(64, N - i0);
  lr_sh_wave_copy<true>(wl, const_cast<float*>(shs) + (size_t)i0 * L, L, rows * L, lane);
  lr_sh_wave_sync();
  const int i = i0 + lane;
  if (i >= N) return;
  float vx = means[3 * i] - campos[0], vy = means[3 * i + 1] - campos[1], vz = means[3 * i + 2] - campos[2];
  const float inv = 1.f / sqrtf(vx * vx + vy * vy + vz * vz);
  const float x = vx * inv, y = vy * inv, z = vz * inv;
  float b[16], bx[16], by[16], bz[16];
  lr_sh_basis(deg, x, y, z, b, bx, by, bz);
  const int nk = (deg + 1) * (deg + 1);
  const float* sh = wl + lane * (L + 1);
  float c[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
  for (int k = 0; k < 16; k++) {
    if (k < nk) {
      c[0] = lr_fma(b[k], sh[3 * k], c[0]); c[1] = lr_fma(b[k], sh[3 * k + 1], c[1]); c[2] = lr_fma(b[k], sh[3 * k + 2], c[2]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    clamped[3 * (size_t)i + ch] = c[ch] < 0.f;
    colors[3 * (size_t)i + ch] = c[ch] < 0.f ? 0.f : c[ch];   // (not fmaxf: a NaN colour stays a NaN)
  }
}

template <bool ACCUMULATE>  // true: g_shs += (running sums over views), false: g_shs = (overwritten)
__global__ void __launch_bounds__(256)
lr_sh_bwd_kernel(int N, int deg, int M, const float* __restrict__ means, const float* __restrict__ campos,
                 const float* __restrict__ shs, const uint8_t* __restrict__ clamped,
                 const float* __restrict__ g_colors, float* __restrict__ g_shs, float* __restrict__ g_means) {
  extern __shared__ float lr_sh_lds[];
  const int L = 3 * M, lane = threadIdx.x & 63;
  float* const wl = lr_sh_lds + (threadIdx.x >> 6) * 64 * (L + 1);
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);
  if (i0 >= N) return;
  const int rows = min(64, N - i0);
  lr_sh_wave_copy<true>(wl, const_cast<float*>(shs) + (size_t)i0 * L, L, rows * L, lane);
  lr_sh_wave_sync();
  const int i = i0 + lane;
  if (i < N) {
    const float vx = means[3 * i] - campos[0], vy = means[3 * i + 1] - campos[1], vz = means[3 * i + 2] - campos[2];
    const float n2 = vx * vx + vy * vy + vz * vz;
    const float inv = 1.f / sqrtf(n2);
    const float x = vx * inv, y = vy * inv, z = vz * inv;
    float b[16], bx[16], by[16], bz[16];
    lr_sh_basis(deg, x, y, z, b, bx, by, bz);
    const int nk = (deg + 1) * (deg + 1);
    float* row = wl + lane * (L + 1);  // coefficients in, their gradients out (each slot is consumed before it is overwritten)
    float g[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) g[ch] = clamped[3 * (size_t)i + ch] ? 0.f : g_colors[3 * (size_t)i + ch];
    float gdx = 0.f, gdy = 0.f, gdz = 0.f;  // dL/d(unit direction)
    for (int k = 0; k < M; k++) {
      if (k < nk) {
        const float s = row[3 * k] * g[0] + row[3 * k + 1] * g[1] + row[3 * k + 2] * g[2];
        row[3 * k] = b[k] * g[0]; row[3 * k + 1] = b[k] * g[1]; row[3 * k + 2] = b[k] * g[2];
        gdx = lr_fma(bx[k], s, gdx); gdy = lr_fma(by[k], s, gdy); gdz = lr_fma(bz[k], s, gdz);
      } else {
        row[3 * k] = 0.f; row[3 * k + 1] = 0.f; row[3 * k + 2] = 0.f;
      }
    }
    // d = v/|v|  ->  dL/dv = (dL/dd - d (d . dL/dd)) / |v|
    const float dot = x * gdx + y * gdy + z * gdz;
    g_means[3 * (size_t)i + 0] += (gdx - x * dot) * inv;
    g_means[3 * (size_t)i + 1] += (gdy - y * dot) * inv;
    g_means[3 * (size_t)i + 2] += (gdz - z * dot) * inv;
  }
  lr_sh_wave_sync();
  lr_sh_wave_copy<false, ACCUMULATE>(wl, g_shs + (size_t)i0 * L, L, rows * L, lane);
}

void lr_launch_sh_fwd(int N, int deg, int M, const float* means, const float* campos, const float* shs, float* colors,
                      uint8_t* clamped, hipStream_t s) {
  if (N <= 0) return;
  const size_t lds = sizeof(float) * 4 * 64 * (size_t)(3 * M + 1);
  hipLaunchKernelGGL(lr_sh_fwd_kernel, dim3((N + 255) / 256), dim3(256), lds, s, N, deg, M, means, campos, shs, colors, clamped);
}
void lr_launch_sh_bwd(int N, int deg, int M, const float* means, const float* campos, const float* shs,
                      const uint8_t* clamped, const float* g_colors, float* g_shs, float* g_means, bool accumulate,
                      hipStream_t s) {
  if (N <= 0) return;
  const size_t lds = sizeof(float) * 4 * 64 * (size_t)(3 * M + 1);
  if (accumulate)
    hipLaunchKernelGGL(lr_sh_bwd_kernel<true>, dim3((N + 255) / 256), dim3(256), lds, s, N, deg, M, means, campos, shs,
                       clamped, g_colors, g_shs, g_means);
  else
    hipLaunchKernelGGL(lr_sh_bwd_kernel<false>, dim3((N + 255) / 256), dim3(256), lds, s, N, deg, M, means, campos, shs,
                       clamped, g_colors, g_shs, g_means);
}

// ---- LoG.get_all + Activation.activate_root_return, fused -------------------------------------
// /root/reference/LoG/model/level_of_gaussian.py:262-296 gathers every model buffer at the selected rows (one
// indexing kernel per key, a cat with the node rows) and /root/reference/LoG/model/activation.py:27-44 activates them
// with ~25 elementwise kernels: exp (scales), sigmoid (opacity), normalize (quaternions), SH2RGB(colors) +
// eval_sh_wobase(dir, shs) (/root/reference/LoG/model/sh_utils.py:31-72).  Here: one kernel gathers the rows, writes
// the raw copies (they become the step's nn.Parameters) and the activated tensors the rasterizer consumes; one kernel
// turns the rasterizer's input gradients into the gradients of the raw copies.
// LoG's SH layout: colors[P,3] is the DC term, shs[P,K,3] the K = (max_degree+1)^2 - 1 higher coefficients, no clamp.

__global__ void __launch_bounds__(256)
ga_fwd_kernel(GatherArgs a) {
  extern __shared__ float lr_sh_lds[];  // 4 waves x (64 rows x (L+1) floats)
  __shared__ int64_t rowid[4][64];
  const int L = 3 * a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);
  if (i0 >= a.n) return;
  const int rows = min(64, a.n - i0);
  const int i = i0 + lane;
  const bool ok = i < a.n;
  int64_t row = ok ? a.index[i] : 0;
  if (row < 0 || row >= a.num_points) row = 0;   // an invalid index reads row 0 instead of faulting
  rowid[wave][lane] = row;
  float p[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
  if (ok) {
    float s[3], q[4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[k] = a.xyz[3 * row + k]; s[k] = a.scaling[3 * row + k]; c[k] = a.colors[3 * row + k];
    }
    const float4 q4 = reinterpret_cast<const float4*>(a.rotation)[row];
    q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
    const float o = a.opacity[row];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a.r_xyz[3 * (size_t)i + k] = p[k]; a.r_scaling[3 * (size_t)i + k] = s[k]; a.r_colors[3 * (size_t)i + k] = c[k];
      a.a_scaling[3 * (size_t)i + k] = expf(s[k]);
    }
    reinterpret_cast<float4*>(a.r_rotation)[i] = q4;
    a.r_opacity[i] = o;
    a.a_opacity[i] = ga_sigmoid(o);
    const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    reinterpret_cast<float4*>(a.a_rotation)[i] = float4{q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm};
  }
  float col[3] = {lr_fma(c[0], SH_C0, 0.5f), lr_fma(c[1], SH_C0, 0.5f), lr_fma(c[2], SH_C0, 0.5f)};   // SH2RGB
  if (L > 0) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    lr_sh_wave_sync();                                      // rowid[] written by this wave
    const uint32_t magic = 0xffffffffu / (uint32_t)a.K + 1u;  // e / K for e < 65536 and K >= 2 (K = 1: 2^32 does not fit)
    float* const out = a.r_shs + (size_t)i0 * L;
    // lanes walk the rows' coefficients contiguously, one (r, g, b) triple = 12 bytes per access (a float at a time this
    // loop was 45 dependent 4-byte gathers per lane at degree 3), four in flight
#pragma unroll 4
    for (int e = lane; e < rows * a.K; e += 64) {
      const int g = a.K == 1 ? e : (int)__umulhi((uint32_t)e, magic), j = e - g * a.K;
      const float* __restrict__ src = a.shs + (size_t)rowid[wave][g] * L + 3 * j;
      const float v0 = src[0], v1 = src[1], v2 = src[2];
      float* o = out + 3 * (size_t)e;                         // the raw copy is contiguous in e
      o[0] = v0; o[1] = v1; o[2] = v2;
      float* w = wl + g * (L + 1) + 3 * j;
      w[0] = v0; w[1] = v1; w[2] = v2;
    }
    lr_sh_wave_sync();
    if (ok && a.deg > 0) {
      const float vx = p[0] - a.campos[0], vy = p[1] - a.campos[1], vz = p[2] - a.campos[2];
      const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
      float b[16], bx[16], by[16], bz[16];
      lr_sh_basis(a.deg, vx / nrm, vy / nrm, vz / nrm, b, bx, by, bz);
      const int nk = (a.deg + 1) * (a.deg + 1);
      const float* sh = wl + lane * (L + 1);
#pragma unroll
      for (int k = 1; k < 16; k++) {
        if (k < nk && k - 1 < a.K) {
          col[0] = lr_fma(b[k], sh[3 * (k - 1)], col[0]); col[1] = lr_fma(b[k], sh[3 * (k - 1) + 1], col[1]);
          col[2] = lr_fma(b[k], sh[3 * (k - 1) + 2], col[2]);
        }
      }
    }
  }
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.a_colors[3 * (size_t)i + k] = col[k];
  }
}


__global__ void __launch_bounds__(256)
ga_bwd_kernel(ActBwdArgs a) {
  extern __shared__ float lr_sh_lds[];
  const int L = 3 * a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);
  if (i0 >= a.n) return;
  const int rows = min(64, a.n - i0);
  const int i = i0 + lane;
  const bool ok = i < a.n;
  float gc[3] = {0.f, 0.f, 0.f};
  if (ok) {
    const size_t c = (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; k++) gc[k] = a.g_a_colors[3 * c + k];
    float g[14];                                            // (g[0..2], dL/dxyz, is not this kernel's: autograd passes it on)
    ga_act_grads(a, c, GA_ALL_KEYS, gc, g);
#pragma unroll
    for (int k = 0; k < 3; k++) { a.g_colors[3 * c + k] = g[6 + k]; a.g_scaling[3 * c + k] = g[3 + k]; }
    a.g_opacity[c] = g[9];
    reinterpret_cast<float4*>(a.g_rotation)[c] = float4{g[10], g[11], g[12], g[13]};
  }
  if (L > 0 && a.g_shs) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    if (ok) ga_sh_grad_row(a, i, gc, wl + lane * (L + 1));
    lr_sh_wave_sync();
    lr_sh_wave_copy<false, false>(wl, a.g_shs + (size_t)i0 * L, L, rows * L, lane);
  }
}

// ---- activation backward + sparse Adam in one kernel (round 6; round-5 verdict, next #6) -------------------------------
// A single-view LoG step runs the activation backward (raw gradients of the selected rows: 59 floats per row at SH degree 3,
// written compact) and, one launch later, SparseOptimizer.step (sparse_optimizer.py:41-78,163-196), which reads those
// gradients back together with the gathered parameters and both moments.  Fused, a raw gradient never leaves the registers /
// the wave's LDS rows: per element the kernel reads the gathered parameter (compact) and both moments (model rows) and
// writes both moments and the model row -- 24 bytes instead of 32 (+ the launch).  The chain rule is ga_bwd_kernel's and the
// update adam_kernel's (counter.hip) -- the same functions of sh_basis.hpp and common.hpp -- so the model and the moments come
// out bit for bit as from the two kernels.
// key order: 0 xyz, 1 scaling, 2 opacity, 3 rotation, 4 colors, 5 shs (model == nullptr: key not optimised).

__global__ void __launch_bounds__(256)
ga_bwd_adam_kernel(ActBwdArgs a, AdamArgs f, const float* __restrict__ g_a_xyz, const int32_t* __restrict__ radii) {
  extern __shared__ float lr_sh_lds[];
  __shared__ long long lr_rowidx[4][64];
  const int L = 3 * a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 256 + (threadIdx.x & ~63);
  if (i0 >= a.n) return;
  const int rows = min(64, a.n - i0);
  const int i = i0 + lane;
  const bool ok = i < a.n;
  float gc[3] = {0.f, 0.f, 0.f};
  long long row = -1;                                       // the model row this lane updates (-1: not visible / no row)
  if (ok && radii[i] > 0) {
    row = f.index[i];
    if (row < 0 || row >= (long long)f.num_points) row = -1;
  }
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; k++) gc[k] = a.g_a_colors[3 * (size_t)i + k];
  }
  {
    // the row's 14 small values; a row that is not visible wants no key: nothing of it is loaded
    const bool vis = row >= 0;
    const size_t r = vis ? (size_t)row : 0, c = ok ? (size_t)i : 0;
    unsigned want = 0;
#pragma unroll
    for (int key = 0; key < 5; key++) want |= (vis && f.key[key].model) ? GA_KEY(key) : 0u;
    float g[14];
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = (want & GA_KEY(0)) ? g_a_xyz[3 * c + k] : 0.f;
    ga_act_grads(a, c, want, gc, g);
    GaElem e[14];
#pragma unroll
    for (int k = 0; k < 14; k++) {
      const GaSmall s = ga_small(k);
      e[k].on = (want & GA_KEY(s.key)) != 0; e[k].o = s.width * r + s.col;
      e[k].p0 = e[k].on ? f.key[s.key].param[s.width * c + s.col] : 0.f;
      e[k].g = g[k];
    }
    // all moments requested, then all updates
#pragma unroll
    for (int k = 0; k < 14; k++) ga_adam_load(f.key[ga_small(k).key], e[k]);
#pragma unroll
    for (int k = 0; k < 14; k++) ga_adam_store(f.key[ga_small(k).key], f, e[k]);
  }
  if (L > 0 && f.key[5].model) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    lr_rowidx[wave][lane] = row;
    if (ok) ga_sh_grad_row(a, i, gc, wl + lane * (L + 1));
    lr_sh_wave_sync();
    // the wave walks its rows' L coefficients contiguously: element e = (row r, column c) of the compact block; the model
    // side is one contiguous 4 L-byte piece per visible row.  GA_SH_UNROLL elements per lane in flight.
    const float* __restrict__ p_sh = f.key[5].param + (size_t)i0 * L;
    const int total = rows * L;
    for (int e0 = lane; e0 < total; e0 += 64 * GA_SH_UNROLL) {
      GaElem e[GA_SH_UNROLL];
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) {
        const int x = e0 + 64 * u;
        e[u].on = false; e[u].o = 0; e[u].p0 = 0.f; e[u].g = 0.f;
        if (x < total) {
          const int r = x / L, c = x - r * L;
          const long long mr = lr_rowidx[wave][r];
          if (mr >= 0) { e[u].on = true; e[u].o = (size_t)mr * L + c; e[u].p0 = p_sh[x]; e[u].g = wl[r * (L + 1) + c]; }
        }
      }
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) ga_adam_load(f.key[5], e[u]);
#pragma unroll
      for (int u = 0; u < GA_SH_UNROLL; u++) ga_adam_store(f.key[5], f, e[u]);
    }
  }
}

hipError_t lr_launch_activate_bwd_adam(const ActBwdArgs& a, const AdamArgs& f, const float* g_a_xyz, const int32_t* radii,
                                       hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  lr_ga_lds_once<ga_bwd_adam_kernel>();
  lr_prof_begin(LRK_ADAM, s);
  hipLaunchKernelGGL(ga_bwd_adam_kernel, dim3((a.n + 255) / 256), dim3(256),
                     (a.K > 0 && f.key[5].model) ? lr_ga_lds_bytes(a.K) : 0, s, a, f, g_a_xyz, radii);
  lr_prof_end(LRK_ADAM, s);
  return hipGetLastError();
}

hipError_t lr_launch_gather_activate(const GatherArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  lr_ga_lds_once<ga_fwd_kernel>();
  lr_ga_lds_once<ga_bwd_kernel>();   // (with the forward, as it always was: the backward's first launch finds it done)
  lr_prof_begin(LRK_GATHER, s);
  hipLaunchKernelGGL(ga_fwd_kernel, dim3((a.n + 255) / 256), dim3(256), a.K > 0 ? lr_ga_lds_bytes(a.K) : 0, s, a);
  lr_prof_end(LRK_GATHER, s);
  return hipGetLastError();
}
hipError_t lr_launch_activate_bwd(const ActBwdArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  lr_ga_lds_once<ga_bwd_kernel>();
  lr_prof_begin(LRK_GATHER_BWD, s);
  hipLaunchKernelGGL(ga_bwd_kernel, dim3((a.n + 255) / 256), dim3(256), (a.K > 0 && a.g_shs) ? lr_ga_lds_bytes(a.K) : 0, s, a);
  lr_prof_end(LRK_GATHER_BWD, s);
  return hipGetLastError();
}
