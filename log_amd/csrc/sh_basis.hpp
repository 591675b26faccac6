// sh_basis.hpp -- the device functions that sh.hip and accumulate.hip share: the SH basis, the wave-level LDS hand-over and
// the two halves of one element's Adam update.  One definition each, so the kernels of both files run the same op sequences.
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

// One element's Adam update (the op sequence of adam_kernel, counter.hip) in two halves, so that a thread can have the
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
  const float m = lr_fma(e.g, f.omb1, e.m0 * f.beta1);
  const float v = lr_fma(f.omb2 * e.g, e.g, e.v0 * f.beta2);
  k.exp_avg[e.o] = m;
  k.exp_avg_sq[e.o] = v;
  float vd = v;
  if (k.max_exp_avg_sq) {
    vd = lr_max_nan(e.vm, v);
    k.max_exp_avg_sq[e.o] = vd;
  }
  const float denom = sqrtf(vd) / f.bc2_sqrt + f.eps;
  k.model[e.o] = e.p0 + k.neg_step_size * (m / denom);
}
