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
#include "sh_basis.hpp"   // lr_sh_basis (reads the two tables above), lr_sh_wave_sync, the Adam element halves

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
#pragma unroll
    for (int k = 0; k < 3; k++) {
      gc[k] = a.g_a_colors[3 * (size_t)i + k];
      a.g_colors[3 * (size_t)i + k] = gc[k] * SH_C0;
      a.g_scaling[3 * (size_t)i + k] = a.g_a_scaling[3 * (size_t)i + k] * expf(a.r_scaling[3 * (size_t)i + k]);
    }
    const float sg = ga_sigmoid(a.r_opacity[i]);
    a.g_opacity[i] = a.g_a_opacity[i] * (sg * (1.f - sg));
    const float4 q = reinterpret_cast<const float4*>(a.r_rotation)[i], gy = reinterpret_cast<const float4*>(a.g_a_rotation)[i];
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w, nrm = sqrtf(n2);
    float4 gq = float4{0.f, 0.f, 0.f, 0.f};
    if (nrm > 1e-12f) {   // y = q / |q|: dL/dq = (g - y (y . g)) / |q|; below eps the clamp makes y = q / eps
      const float ix = 1.f / nrm, yx = q.x * ix, yy = q.y * ix, yz = q.z * ix, yw = q.w * ix;
      const float dot = yx * gy.x + yy * gy.y + yz * gy.z + yw * gy.w;
      gq = float4{(gy.x - yx * dot) * ix, (gy.y - yy * dot) * ix, (gy.z - yz * dot) * ix, (gy.w - yw * dot) * ix};
    } else {
      gq = float4{gy.x * 1e12f, gy.y * 1e12f, gy.z * 1e12f, gy.w * 1e12f};
    }
    reinterpret_cast<float4*>(a.g_rotation)[i] = gq;
  }
  if (L > 0 && a.g_shs) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    if (ok) {
      float b[16], bx[16], by[16], bz[16];
#pragma unroll
      for (int k = 0; k < 16; k++) b[k] = 0.f;
      if (a.deg > 0) {
        const float vx = a.r_xyz[3 * (size_t)i] - a.campos[0], vy = a.r_xyz[3 * (size_t)i + 1] - a.campos[1],
                    vz = a.r_xyz[3 * (size_t)i + 2] - a.campos[2];
        const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
        lr_sh_basis(a.deg, vx / nrm, vy / nrm, vz / nrm, b, bx, by, bz);
      }
      const int nk = (a.deg + 1) * (a.deg + 1);
      float* rowp = wl + lane * (L + 1);
      for (int k = 0; k < a.K; k++) {
        const float w = (k + 1 < nk && k + 1 < 16) ? b[k + 1] : 0.f;   // coefficients above the active degree: zero gradient
        rowp[3 * k] = w * gc[0]; rowp[3 * k + 1] = w * gc[1]; rowp[3 * k + 2] = w * gc[2];
      }
    }
    lr_sh_wave_sync();
    lr_sh_wave_copy<false, false>(wl, a.g_shs + (size_t)i0 * L, L, rows * L, lane);
  }
}

// ---- activation backward + sparse Adam in one kernel (round 6; round-5 verdict, next #6) -------------------------------
// A single-view LoG step runs the activation backward (raw gradients of the selected rows: 59 floats per row at SH degree 3,
// written compact) and, one launch later, SparseOptimizer.step (sparse_optimizer.py:41-78,163-196), which reads those
// gradients back together with the gathered parameters and both moments.  Fused, a raw gradient never leaves the registers /
// the wave's LDS rows: per element the kernel reads the gathered parameter (compact) and both moments (model rows) and
// writes both moments and the model row -- 24 bytes instead of 32 (+ the launch).  Same op sequences as ga_bwd_kernel and
// adam_kernel (counter.hip), so the model and the moments come out bit for bit as from the two kernels.
// key order: 0 xyz, 1 scaling, 2 opacity, 3 rotation, 4 colors, 5 shs (model == nullptr: key not optimised).

#define GA_SH_UNROLL 8
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
    // the row's 14 small values: xyz 0-2, scaling 3-5, colors 6-8, opacity 9, rotation 10-13 (keys 0, 1, 4, 2, 3)
    const bool vis = row >= 0;
    const size_t r = vis ? (size_t)row : 0, c = ok ? (size_t)i : 0;
    GaElem e[14];
    float4 q = {0.f, 0.f, 0.f, 1.f}, gy = {0.f, 0.f, 0.f, 0.f};
    if (vis && f.key[3].model) { q = reinterpret_cast<const float4*>(a.r_rotation)[c]; gy = reinterpret_cast<const float4*>(a.g_a_rotation)[c]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      e[k].on = vis && f.key[0].model; e[k].o = 3 * r + k;
      e[k].p0 = e[k].on ? f.key[0].param[3 * c + k] : 0.f;
      e[k].g = e[k].on ? g_a_xyz[3 * c + k] : 0.f;
      e[3 + k].on = vis && f.key[1].model; e[3 + k].o = 3 * r + k;
      e[3 + k].p0 = e[3 + k].on ? f.key[1].param[3 * c + k] : 0.f;
      e[3 + k].g = e[3 + k].on ? a.g_a_scaling[3 * c + k] * expf(a.r_scaling[3 * c + k]) : 0.f;
      e[6 + k].on = vis && f.key[4].model; e[6 + k].o = 3 * r + k;
      e[6 + k].p0 = e[6 + k].on ? f.key[4].param[3 * c + k] : 0.f;
      e[6 + k].g = gc[k] * SH_C0;
    }
    e[9].on = vis && f.key[2].model; e[9].o = r;
    e[9].p0 = e[9].on ? f.key[2].param[c] : 0.f;
    e[9].g = 0.f;
    if (e[9].on) {
      const float sg = ga_sigmoid(a.r_opacity[c]);
      e[9].g = a.g_a_opacity[c] * (sg * (1.f - sg));
    }
    {
      const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w, nrm = sqrtf(n2);
      float4 gq;
      if (nrm > 1e-12f) {   // y = q / |q|: dL/dq = (g - y (y . g)) / |q|; below eps the clamp makes y = q / eps
        const float ix = 1.f / nrm, yx = q.x * ix, yy = q.y * ix, yz = q.z * ix, yw = q.w * ix;
        const float dot = yx * gy.x + yy * gy.y + yz * gy.z + yw * gy.w;
        gq = float4{(gy.x - yx * dot) * ix, (gy.y - yy * dot) * ix, (gy.z - yz * dot) * ix, (gy.w - yw * dot) * ix};
      } else {
        gq = float4{gy.x * 1e12f, gy.y * 1e12f, gy.z * 1e12f, gy.w * 1e12f};
      }
      const float gqa[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        e[10 + k].on = vis && f.key[3].model; e[10 + k].o = 4 * r + k;
        e[10 + k].p0 = e[10 + k].on ? f.key[3].param[4 * c + k] : 0.f;
        e[10 + k].g = gqa[k];
      }
    }
    // all moments requested, then all updates
#pragma unroll
    for (int k = 0; k < 14; k++) ga_adam_load(f.key[k < 3 ? 0 : (k < 6 ? 1 : (k < 9 ? 4 : (k < 10 ? 2 : 3)))], e[k]);
#pragma unroll
    for (int k = 0; k < 14; k++) ga_adam_store(f.key[k < 3 ? 0 : (k < 6 ? 1 : (k < 9 ? 4 : (k < 10 ? 2 : 3)))], f, e[k]);
  }
  if (L > 0 && f.key[5].model) {
    float* const wl = lr_sh_lds + wave * 64 * (L + 1);
    lr_rowidx[wave][lane] = row;
    if (ok) {
      float b[16], bx[16], by[16], bz[16];
#pragma unroll
      for (int k = 0; k < 16; k++) b[k] = 0.f;
      if (a.deg > 0) {
        const float vx = a.r_xyz[3 * (size_t)i] - a.campos[0], vy = a.r_xyz[3 * (size_t)i + 1] - a.campos[1],
                    vz = a.r_xyz[3 * (size_t)i + 2] - a.campos[2];
        const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
        lr_sh_basis(a.deg, vx / nrm, vy / nrm, vz / nrm, b, bx, by, bz);
      }
      const int nk = (a.deg + 1) * (a.deg + 1);
      float* rowp = wl + lane * (L + 1);
      for (int k = 0; k < a.K; k++) {
        const float w = (k + 1 < nk && k + 1 < 16) ? b[k + 1] : 0.f;   // coefficients above the active degree: zero gradient
        rowp[3 * k] = w * gc[0]; rowp[3 * k + 1] = w * gc[1]; rowp[3 * k + 2] = w * gc[2];
      }
    }
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
  const size_t lds = sizeof(float) * 4 * 64 * (size_t)(3 * a.K + 1);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_bwd_adam_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_set = true;
  }
  lr_prof_begin(LRK_ADAM, s);
  hipLaunchKernelGGL(ga_bwd_adam_kernel, dim3((a.n + 255) / 256), dim3(256), (a.K > 0 && f.key[5].model) ? lds : 0, s, a, f,
                     g_a_xyz, radii);
  lr_prof_end(LRK_ADAM, s);
  return hipGetLastError();
}

hipError_t lr_launch_gather_activate(const GatherArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const size_t lds = sizeof(float) * 4 * 64 * (size_t)(3 * a.K + 1);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_set = true;
  }
  lr_prof_begin(LRK_GATHER, s);
  hipLaunchKernelGGL(ga_fwd_kernel, dim3((a.n + 255) / 256), dim3(256), a.K > 0 ? lds : 0, s, a);
  lr_prof_end(LRK_GATHER, s);
  return hipGetLastError();
}
hipError_t lr_launch_activate_bwd(const ActBwdArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const size_t lds = sizeof(float) * 4 * 64 * (size_t)(3 * a.K + 1);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_set = true;
  }
  lr_prof_begin(LRK_GATHER_BWD, s);
  hipLaunchKernelGGL(ga_bwd_kernel, dim3((a.n + 255) / 256), dim3(256), (a.K > 0 && a.g_shs) ? lds : 0, s, a);
  lr_prof_end(LRK_GATHER_BWD, s);
  return hipGetLastError();
}
