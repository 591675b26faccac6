// sh_basis.hpp -- what the row kernels of sh.hip and accumulate.hip share, one definition each, so that the kernels of both
// files run the same op sequences (the tests hold them bit for bit against each other):
//   * lr_sh_basis, lr_sh_wave_sync      : the SH basis and the wave-level LDS hand-over
//   * ga_small                          : element k of a row's 14 small values -> (key, column, key width)
//   * ga_quat_grad, ga_act_grads        : the activation chain rule of those values (ga_bwd_kernel, ga_bwd_adam_kernel,
//                                         acc_bwd_kernel: each keeps only where the 14 values go)
//   * ga_sh_grad_row                    : the SH gradients of one row, written into the lane's LDS row (the same three)
//   * ga_adam_load, ga_adam_store       : the two halves of one element's Adam update around lr_adam_elem (common.hpp;
//                                         ga_bwd_adam_kernel, acc_adam_kernel)
//   * lr_ga_lds_bytes, lr_ga_lds_once   : the launchers' dynamic-LDS size and its attribute call
// The including file defines the coefficient tables kC2[5] and kC3[7] in __constant__ memory, then LR_SH_TABLES_DEFINED, BEFORE this header (sh.hip with
// external linkage, as it always had them; any other file `static`): a table defined here would have to be static or inline
// in every file, and sh.hip's device code is kept as it was, symbol for symbol.
#pragma once
#include "common.hpp"
#ifndef LR_SH_TABLES_DEFINED
#error "sh_basis.hpp: define the __constant__ tables kC2[5] and kC3[7], then LR_SH_TABLES_DEFINED, before including this header"
#endif

#define SH_C0 0.28209479177387814f
#define SH_C1 0.4886025119029199f

// basis values b[0..15] and their partial derivatives w.r.t. the unit direction (x,y,z)
LR_DEV void lr_sh_basis(int deg, float x, float y, float z, float b[16], float bx[16], float by[16], float bz[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) { b[k] = 0.f; bx[k] = 0.f; by[k] = 0.f; bz[k] = 0.f; }
  b[0] = SH_C0;
  if (deg > 0) {
    b[1] = -SH_C1 * y; by[1] = -SH_C1;
    b[2] = SH_C1 * z; bz[2] = SH_C1;
    b[3] = -SH_C1 * x; bx[3] = -SH_C1;
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      b[4] = kC2[0] * xy; bx[4] = kC2[0] * y; by[4] = kC2[0] * x;
      b[5] = kC2[1] * yz; by[5] = kC2[1] * z; bz[5] = kC2[1] * y;
      b[6] = kC2[2] * (2.f * zz - xx - yy); bx[6] = -2.f * kC2[2] * x; by[6] = -2.f * kC2[2] * y; bz[6] = 4.f * kC2[2] * z;
      b[7] = kC2[3] * xz; bx[7] = kC2[3] * z; bz[7] = kC2[3] * x;
      b[8] = kC2[4] * (xx - yy); bx[8] = 2.f * kC2[4] * x; by[8] = -2.f * kC2[4] * y;
      if (deg > 2) {
        b[9] = kC3[0] * y * (3.f * xx - yy); bx[9] = kC3[0] * 6.f * xy; by[9] = kC3[0] * (3.f * xx - 3.f * yy);
        b[10] = kC3[1] * xy * z; bx[10] = kC3[1] * yz; by[10] = kC3[1] * xz; bz[10] = kC3[1] * xy;
        b[11] = kC3[2] * y * (4.f * zz - xx - yy); bx[11] = -2.f * kC3[2] * xy;
        by[11] = kC3[2] * (4.f * zz - xx - 3.f * yy); bz[11] = 8.f * kC3[2] * yz;
        b[12] = kC3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); bx[12] = -6.f * kC3[3] * xz; by[12] = -6.f * kC3[3] * yz;
        bz[12] = kC3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
        b[13] = kC3[4] * x * (4.f * zz - xx - yy); bx[13] = kC3[4] * (4.f * zz - 3.f * xx - yy);
        by[13] = -2.f * kC3[4] * xy; bz[13] = 8.f * kC3[4] * xz;
        b[14] = kC3[5] * z * (xx - yy); bx[14] = 2.f * kC3[5] * xz; by[14] = -2.f * kC3[5] * yz; bz[14] = kC3[5] * (xx - yy);
        b[15] = kC3[6] * x * (xx - 3.f * yy); bx[15] = kC3[6] * (3.f * xx - 3.f * yy); by[15] = -6.f * kC3[6] * xy;
      }
    }
  }
}

LR_DEV void lr_sh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One element's Adam update (lr_adam_elem, common.hpp: what adam_kernel runs) in two halves, so that a thread can have the
// moments of ALL its elements in flight before the first store (written as one read-modify-write after the other, every
// store may alias the next load -- the moments arrive as plain float* -- and a lane's 14 + 3 K elements become one
// dependent chain of memory round trips).
struct GaElem { size_t o; float p0, g, m0, v0, vm; bool on; };
LR_DEV void ga_adam_load(const AdamKey& k, GaElem& e) {
  e.m0 = 0.f; e.v0 = 0.f; e.vm = 0.f;
  if (e.on) {
    e.m0 = k.exp_avg[e.o];
    e.v0 = k.exp_avg_sq[e.o];
    if (k.max_exp_avg_sq) e.vm = k.max_exp_avg_sq[e.o];
  }
}
LR_DEV void ga_adam_store(const AdamKey& k, const AdamArgs& f, const GaElem& e) {
  if (!e.on) return;
  const LrAdamElem r = lr_adam_elem(e.g, e.m0, e.v0, e.vm, k.max_exp_avg_sq != nullptr, f.beta1, f.beta2, f.omb1, f.omb2,
                                    f.bc2_sqrt, f.eps, k.neg_step_size, e.p0);
  k.exp_avg[e.o] = r.m;
  k.exp_avg_sq[e.o] = r.v;
  if (k.max_exp_avg_sq) k.max_exp_avg_sq[e.o] = r.vd;
  k.model[e.o] = r.p;
}

// ---- a row's 14 small values -------------------------------------------------------------------------------------------
// Key order everywhere: 0 xyz, 1 scaling, 2 opacity, 3 rotation, 4 colors, 5 shs; GA_KEY(i) is key i's bit in a mask of wanted
// keys.  A lane holds its row's small values as xyz 0-2, scaling 3-5, colours 6-8, opacity 9, rotation 10-13.
#define GA_KEY(i) (1u << (i))
#define GA_ALL_KEYS 0x3fu
#define GA_SH_UNROLL 8   // elements per lane in flight in the contiguous SH walks of the step kernels
struct GaSmall { int key, col, width; };
LR_DEV constexpr GaSmall ga_small(int k) {
  constexpr int key[14] = {0, 0, 0, 1, 1, 1, 4, 4, 4, 2, 3, 3, 3, 3}, col[14] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 3};
  constexpr int width[14] = {3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 4, 4, 4, 4};
  return GaSmall{key[k], col[k], width[k]};
}

// y = q / max(|q|, 1e-12):  dL/dq = (g - y (y . g)) / |q|; below eps the clamp makes y = q / eps
LR_DEV float4 ga_quat_grad(float4 q, float4 gy) {
  const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w, nrm = sqrtf(n2);
  if (nrm > 1e-12f) {
    const float ix = 1.f / nrm, yx = q.x * ix, yy = q.y * ix, yz = q.z * ix, yw = q.w * ix;
    const float dot = yx * gy.x + yy * gy.y + yz * gy.z + yw * gy.w;
    return float4{(gy.x - yx * dot) * ix, (gy.y - yy * dot) * ix, (gy.z - yz * dot) * ix, (gy.w - yw * dot) * ix};
  }
  return float4{gy.x * 1e12f, gy.y * 1e12f, gy.z * 1e12f, gy.w * 1e12f};
}

// The activation chain rule of compact row c: g[3..13] = dL/d(raw scaling, colours, opacity, rotation) in the layout above
// (scaling . exp, colours . SH_C0, opacity . s (1 - s), the normalisation's gradient).  gc = the row's dL/d(activated colours),
// which the caller holds for the SH gradients anyway.  A key outside `want` is not loaded and comes out as zero; g[0..2]
// (dL/dxyz, passed through) is the caller's.
LR_DEV void ga_act_grads(const ActBwdArgs& a, size_t c, unsigned want, const float gc[3], float g[14]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    g[3 + k] = (want & GA_KEY(1)) ? a.g_a_scaling[3 * c + k] * expf(a.r_scaling[3 * c + k]) : 0.f;
    g[6 + k] = gc[k] * SH_C0;
  }
  g[9] = 0.f;
  if (want & GA_KEY(2)) {
    const float sg = ga_sigmoid(a.r_opacity[c]);
    g[9] = a.g_a_opacity[c] * (sg * (1.f - sg));
  }
  float4 q = {0.f, 0.f, 0.f, 1.f}, gy = {0.f, 0.f, 0.f, 0.f};
  if (want & GA_KEY(3)) { q = reinterpret_cast<const float4*>(a.r_rotation)[c]; gy = reinterpret_cast<const float4*>(a.g_a_rotation)[c]; }
  const float4 gq = ga_quat_grad(q, gy);
  g[10] = gq.x; g[11] = gq.y; g[12] = gq.z; g[13] = gq.w;
}

// The SH gradients of compact row i: basis_k(direction) * gc for the K stored coefficients, into the lane's LDS row
LR_DEV void ga_sh_grad_row(const ActBwdArgs& a, int i, const float gc[3], float* rowp) {
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
  for (int k = 0; k < a.K; k++) {
    const float w = (k + 1 < nk && k + 1 < 16) ? b[k + 1] : 0.f;   // coefficients above the active degree: zero gradient
    rowp[3 * k] = w * gc[0]; rowp[3 * k + 1] = w * gc[1]; rowp[3 * k + 2] = w * gc[2];
  }
}

// ---- the launchers' dynamic LDS: 4 waves x 64 rows x (3 K + 1) floats --------------------------------------------------------
inline size_t lr_ga_lds_bytes(int K) { return sizeof(float) * 4 * 64 * (size_t)(3 * K + 1); }
template <auto KERNEL>
inline void lr_ga_lds_once() {   // one attribute call per kernel and process
  static bool set = false;
  if (!set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    set = true;
  }
}
