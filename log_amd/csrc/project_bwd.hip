// project_bwd.hip -- A6b: per-Gaussian chain rule from (dL/d ndc-mean, dL/d conic) back to
// means3D / scales / rotations.  Streaming, one thread per Gaussian; everything (cov3D, EWA Jacobian)
// is recomputed from the original inputs instead of being stored by the forward (saves 24+ B/Gaussian
// of HBM traffic each way).  Conventions: SURVEY.md Appendix B; the alpha cap and the 0.1 floor in the
// radius formula carry no gradient; the fork's max(.,0.3) low-pass has the standard sub-gradient.
#include "common.hpp"
#include "launch.hpp"

// TOUCHED (lograst_backward with a point_weight array): a Gaussian whose forward blend weight stayed 0 contributed
// to no pixel, so the reverse walk added nothing to its dL/dmean2D and dL/dconic -- both are exactly zero and so is
// everything the chain rule would compute from them.  Such rows are skipped without reading their 56 input bytes or
// their accumulators (whose conic part the forward then does not zero-fill: the compositing kernel clears the rows it meets) and without the 80-byte read-modify-
// write of the running sums: in an opaque scene most Gaussians are hidden (30 M random Gaussians at opacity 0.999:
// the kernel went from 0.83 ms, at the copy rate, to the touched rows' share).
// The chain rule of ONE Gaussian the forward composited (gm, gs, gq, and dL/dcov3D written / added in place when COV).
#define LR_CAM_SUMS 24
// CAM: the row's terms of dL/dviewmatrix and dL/dprojmatrix, added into cam[LR_CAM_SUMS] (layout: lr_camera_finish_kernel).
// The chain rule once more, in DOUBLE, as far as the camera needs it (no dL/dSigma -> scales / rotations part).  The fp32
// chain above is ill-conditioned for needle-shaped Gaussians (det = a c - b^2 and the quadratic forms in dL/dconic cancel): a
// Gaussian's own gradients carry that error to its own row, but the camera sums add the rows of ALL Gaussians into 24 numbers
// that are ~10x smaller than the sum of the terms' magnitudes, and the rows' fp32 errors do not cancel with them -- on a
// 1024-Gaussian test scene the fp32 terms put dL/dviewmatrix 3e-4 from the float64 reference, these 1e-5 (what the fp32
// forward's decisions leave).  The reverse walk's fp32 sums are not the problem: they enter linearly.  The per-Gaussian
// outputs keep the fp32 chain and its bits.  V and P are row-major in the row-vector convention: t_k = sum_j p_j V[j][k] +
// V[3][k], T0[j] = J00 V[j][0] + J02 V[j][2], T1[j] = J11 V[j][1] + J12 V[j][2], hom_c = sum_j p_j P[j][c] + P[3][c]; dL/dt is
// taken behind the clamp branches (a clamped axis has J02 = -fx ux / tz: no t.x in it), so the J terms are the direct partials
// in V.  Column 3 of V and column 2 of P reach no output: structural zeros, not summed.
LR_DEV void lr_camera_row(const LrView& v, const float pf[3], const float sf[3], const float qf[4], float gnx, float gny,
                          float gA, float gB, float gC, float* cam) {
  const float* __restrict__ Vf = v.view;
  const float* __restrict__ Pf = v.proj;
  double V[12];   // rows 0..3, columns 0..2
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 3; k++) V[3 * j + k] = (double)Vf[4 * j + k];
  const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
  const double r = qf[0], x = qf[1], y = qf[2], z = qf[3];
  const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
                       2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
                       2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)};
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) M[3 * i + k] = R[3 * i + k] * (double)sf[k];
  double S3[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) S3[3 * i + k] = M[3 * i] * M[3 * k] + M[3 * i + 1] * M[3 * k + 1] + M[3 * i + 2] * M[3 * k + 2];
  double t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = p[0] * V[k] + p[1] * V[3 + k] + p[2] * V[6 + k] + V[9 + k];
  const double fx = v.fx, fy = v.fy, tz = t[2], tz2 = tz * tz, tz3 = tz2 * tz;
  const double limx = 1.3 * (double)v.tanfovx, limy = 1.3 * (double)v.tanfovy;
  const double txtz = t[0] / tz, tytz = t[1] / tz;
  const bool cx = (txtz < -limx) || (txtz > limx), cy = (tytz < -limy) || (tytz > limy);
  const double ux = fmin(limx, fmax(-limx, txtz)), uy = fmin(limy, fmax(-limy, tytz));
  const double txc = ux * tz, tyc = uy * tz;
  const double j00 = fx / tz, j02 = -(fx * txc) / tz2, j11 = fy / tz, j12 = -(fy * tyc) / tz2;
  double T0[3], T1[3], ts0[3], ts1[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    T0[j] = j00 * V[3 * j] + j02 * V[3 * j + 2];
    T1[j] = j11 * V[3 * j + 1] + j12 * V[3 * j + 2];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    ts0[k] = T0[0] * S3[k] + T0[1] * S3[3 + k] + T0[2] * S3[6 + k];
    ts1[k] = T1[0] * S3[k] + T1[1] * S3[3 + k] + T1[2] * S3[6 + k];
  }
  const double a_raw = ts0[0] * T0[0] + ts0[1] * T0[1] + ts0[2] * T0[2];
  const double b = ts0[0] * T1[0] + ts0[1] * T1[1] + ts0[2] * T1[2];
  const double c_raw = ts1[0] * T1[0] + ts1[1] * T1[1] + ts1[2] * T1[2];
  double a = a_raw, c = c_raw;
  if (v.filter_mode == LOGRAST_FILTER_DILATE) { a += (double)0.3f; c += (double)0.3f; }   // (the forward's fp32 constant)
  else if (v.filter_mode == LOGRAST_FILTER_CLAMP) { a = fmax(a, (double)0.3f); c = fmax(c, (double)0.3f); }
  const double det = a * c - b * b, di2 = 1.0 / (det * det);
  const double dA = gA, dB = gB, dC = gC;
  double ga = di2 * (-c * c * dA + b * c * dB - b * b * dC);
  const double gb = di2 * (2.0 * b * c * dA - (det + 2.0 * b * b) * dB + 2.0 * a * b * dC);
  double gc = di2 * (-b * b * dA + a * b * dB - a * a * dC);
  if (v.filter_mode == LOGRAST_FILTER_CLAMP) {
    if (!(a_raw >= (double)0.3f)) ga = 0.0;
    if (!(c_raw >= (double)0.3f)) gc = 0.0;
  }
  const double hb = 0.5 * gb;
  double gT0[3], gT1[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    gT0[k] = 2.0 * (ga * ts0[k] + hb * ts1[k]);
    gT1[k] = 2.0 * (hb * ts0[k] + gc * ts1[k]);
  }
  double gj00 = 0.0, gj02 = 0.0, gj11 = 0.0, gj12 = 0.0;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    gj00 += gT0[j] * V[3 * j]; gj02 += gT0[j] * V[3 * j + 2];
    gj11 += gT1[j] * V[3 * j + 1]; gj12 += gT1[j] * V[3 * j + 2];
  }
  const double g_txc = -fx / tz2 * gj02, g_tyc = -fy / tz2 * gj12;
  double g_tz = -fx / tz2 * gj00 - fy / tz2 * gj11 + 2.0 * fx * txc / tz3 * gj02 + 2.0 * fy * tyc / tz3 * gj12;
  double g_tx, g_ty;
  if (cx) { g_tx = 0.0; g_tz += ux * g_txc; } else { g_tx = g_txc; }
  if (cy) { g_ty = 0.0; g_tz += uy * g_tyc; } else { g_ty = g_tyc; }
  // centre path: ndc = h.xy / (h.w + eps)
  const double hx = p[0] * (double)Pf[0] + p[1] * (double)Pf[4] + p[2] * (double)Pf[8] + (double)Pf[12];
  const double hy = p[0] * (double)Pf[1] + p[1] * (double)Pf[5] + p[2] * (double)Pf[9] + (double)Pf[13];
  const double hw = p[0] * (double)Pf[3] + p[1] * (double)Pf[7] + p[2] * (double)Pf[11] + (double)Pf[15];
  const double pw = 1.0 / (hw + 0.0000001);
  const double ghx = (double)gnx * pw, ghy = (double)gny * pw, ghw = -((double)gnx * hx + (double)gny * hy) * pw * pw;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    cam[3 * j + 0] += (float)(j00 * gT0[j] + p[j] * g_tx);
    cam[3 * j + 1] += (float)(j11 * gT1[j] + p[j] * g_ty);
    cam[3 * j + 2] += (float)(j02 * gT0[j] + j12 * gT1[j] + p[j] * g_tz);
    cam[12 + 3 * j + 0] += (float)(p[j] * ghx); cam[12 + 3 * j + 1] += (float)(p[j] * ghy); cam[12 + 3 * j + 2] += (float)(p[j] * ghw);
  }
  cam[9] += (float)g_tx; cam[10] += (float)g_ty; cam[11] += (float)g_tz;
  cam[21] += (float)ghx; cam[22] += (float)ghy; cam[23] += (float)ghw;
}
template <bool ACCUMULATE, bool COV>
LR_DEV void lr_project_bwd_row(const LrView& v, int i, const float* __restrict__ means, const float* __restrict__ scales,
                               const float* __restrict__ rots, float gnx, float gny, float gA, float gB, float gC,
                               float gm[3], float gs[3], float gq[4]) {
  const float* __restrict__ V = v.view;
  const float* __restrict__ Pm = v.proj;
  float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
  float s[3] = {0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  float R[9], Sg[6];
  if (COV) {   // cov3D_precomp (the view carries n x 6 covariances): the chain stops at dL/dSigma
#pragma unroll
    for (int k = 0; k < 6; k++) Sg[k] = v.cov3d[6 * (size_t)i + k];
  } else {
    s[0] = scales[3 * i] * v.scale_modifier; s[1] = scales[3 * i + 1] * v.scale_modifier;
    s[2] = scales[3 * i + 2] * v.scale_modifier;
    const float4 q4 = reinterpret_cast<const float4*>(rots)[i];
    q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
    lr_cov3d(s, q, R, Sg);
  }
  LrEwa e;
  lr_ewa(p, Sg, V, v.fx, v.fy, v.tanfovx, v.tanfovy, v.filter_mode, e);
  const float a = e.a, b = e.b, c = e.c;
  const float det = a * c - b * b;
  const float di2 = 1.f / (det * det);
  // conic = (c, -b, a) / det
  float ga = di2 * (-c * c * gA + b * c * gB - b * b * gC);
  float gb = di2 * (2.f * b * c * gA - (det + 2.f * b * b) * gB + 2.f * a * b * gC);
  float gc = di2 * (-b * b * gA + a * b * gB - a * a * gC);
  if (v.filter_mode == LOGRAST_FILTER_CLAMP) {
    if (!(e.a_raw >= 0.3f)) ga = 0.f;
    if (!(e.c_raw >= 0.3f)) gc = 0.f;
  }
  const float hb = 0.5f * gb;
  // dL/dSigma = T^T G2 T
  float gS[9];
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int k = 0; k < 3; k++)
      gS[3 * j + k] = ga * e.T0[j] * e.T0[k] + hb * (e.T0[j] * e.T1[k] + e.T1[j] * e.T0[k]) + gc * e.T1[j] * e.T1[k];
  // dL/dT = 2 G2 T Sigma
  const float S3[9] = {Sg[0], Sg[1], Sg[2], Sg[1], Sg[3], Sg[4], Sg[2], Sg[4], Sg[5]};
  float gT0[3], gT1[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float ts0 = e.T0[0] * S3[k] + e.T0[1] * S3[3 + k] + e.T0[2] * S3[6 + k];
    float ts1 = e.T1[0] * S3[k] + e.T1[1] * S3[3 + k] + e.T1[2] * S3[6 + k];
    gT0[k] = 2.f * (ga * ts0 + hb * ts1);
    gT1[k] = 2.f * (hb * ts0 + gc * ts1);
  }
  float gj00 = 0.f, gj02 = 0.f, gj11 = 0.f, gj12 = 0.f;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    gj00 += gT0[j] * V[4 * j + 0]; gj02 += gT0[j] * V[4 * j + 2];
    gj11 += gT1[j] * V[4 * j + 1]; gj12 += gT1[j] * V[4 * j + 2];
  }
  const float tz = e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
  const float g_txc = -v.fx / tz2 * gj02, g_tyc = -v.fy / tz2 * gj12;
  float g_tz = -v.fx / tz2 * gj00 - v.fy / tz2 * gj11 + 2.f * v.fx * e.txc / tz3 * gj02 +
               2.f * v.fy * e.tyc / tz3 * gj12;
  float g_tx, g_ty;
  if (e.cx) { g_tx = 0.f; g_tz += e.ux * g_txc; } else { g_tx = g_txc; }
  if (e.cy) { g_ty = 0.f; g_tz += e.uy * g_tyc; } else { g_ty = g_tyc; }
  float m0 = V[0] * g_tx + V[1] * g_ty + V[2] * g_tz;
  float m1 = V[4] * g_tx + V[5] * g_ty + V[6] * g_tz;
  float m2 = V[8] * g_tx + V[9] * g_ty + V[10] * g_tz;
  // centre path: ndc = h.xy / (h.w + eps)
  const float hx = lr_dot3p(Pm[0], Pm[4], Pm[8], p[0], p[1], p[2], Pm[12]);
  const float hy = lr_dot3p(Pm[1], Pm[5], Pm[9], p[0], p[1], p[2], Pm[13]);
  const float hw = lr_dot3p(Pm[3], Pm[7], Pm[11], p[0], p[1], p[2], Pm[15]);
  const float pw = 1.0f / (hw + 0.0000001f);
  const float ghx = gnx * pw, ghy = gny * pw, ghw = -(gnx * hx + gny * hy) * pw * pw;
  m0 += Pm[0] * ghx + Pm[1] * ghy + Pm[3] * ghw;
  m1 += Pm[4] * ghx + Pm[5] * ghy + Pm[7] * ghw;
  m2 += Pm[8] * ghx + Pm[9] * ghy + Pm[11] * ghw;
  gm[0] = m0; gm[1] = m1; gm[2] = m2;
  if (COV) {
    // the six stored entries; an off-diagonal one stands for both symmetric positions of Sigma (the upstream backward's
    // "off-diagonal elements appear twice" rule)
    const float g6[6] = {gS[0], 2.f * gS[1], 2.f * gS[2], gS[4], 2.f * gS[5], gS[8]};
    float* __restrict__ o = v.g_cov3d + 6 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = ACCUMULATE ? o[k] + g6[k] : g6[k];
  } else {
  // Sigma = M M^T, M_ik = R_ik s_k
  float M[9], gM[9], gR[9];
#pragma unroll
  for (int ii = 0; ii < 3; ii++)
#pragma unroll
    for (int k = 0; k < 3; k++) M[3 * ii + k] = R[3 * ii + k] * s[k];
#pragma unroll
  for (int ii = 0; ii < 3; ii++)
#pragma unroll
    for (int k = 0; k < 3; k++)
      gM[3 * ii + k] = 2.f * (gS[3 * ii + 0] * M[0 + k] + gS[3 * ii + 1] * M[3 + k] + gS[3 * ii + 2] * M[6 + k]);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    gs[k] = v.scale_modifier * (gM[k] * R[k] + gM[3 + k] * R[3 + k] + gM[6 + k] * R[6 + k]);
#pragma unroll
    for (int ii = 0; ii < 3; ii++) gR[3 * ii + k] = gM[3 * ii + k] * s[k];
  }
  const float r = q[0], x = q[1], y = q[2], z = q[3];
  gq[0] = 2.f * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
  gq[1] = 2.f * (y * gR[1] + z * gR[2] + y * gR[3] - 2.f * x * gR[4] - r * gR[5] + z * gR[6] + r * gR[7] - 2.f * x * gR[8]);
  gq[2] = 2.f * (-2.f * y * gR[0] + x * gR[1] + r * gR[2] + x * gR[3] + z * gR[5] - r * gR[6] + z * gR[7] - 2.f * y * gR[8]);
  gq[3] = 2.f * (-2.f * z * gR[0] - r * gR[1] + x * gR[2] + r * gR[3] - 2.f * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
  }
}

// The chain rule of ONE live Gaussian i: reads its accumulator row (AOS) or its (dL/dmean2D, dL/dconic) pair, hands out
// the per-view outputs and writes / adds the gradients (see lr_project_bwd_kernel for the template flags).
template <bool ACCUMULATE, bool COV, bool AOS, bool SINKROWS, bool AUXO = false, bool CAM = false, bool ABSO = false>
// (No __restrict__ here: the kernels' own parameters carry it.  Repeated on this inlined function it gave the scheduler
// licence to hoist every load of the row above the chain rule -- 136 -> 170 VGPRs, three waves per SIMD -> two, the
// 30 M-row launch 402 -> 477 us.)
LR_DEV void lr_pbwd_live_row(const LrView& v, int i, const float* means, const float* scales, const float* rots,
                             const float* g_mean2d, const float* g_conic, const float4* rows, float* o_mean2d,
                             float* o_opac, float* o_col, float* g_means3d, float* g_scales, float* g_rots,
                             float* m2d_slice = nullptr, int slice_base = 0, bool staged = false, float* o_aux = nullptr,
                             float* cam = nullptr, float* o_abs = nullptr) {
    float gm[3], gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
    float gnx, gny, gA, gB, gC;
    float gA2 = 0.f, gB2 = 0.f, gC2 = 0.f;   // (AUXO)
    // running sums (ACCUMULATE): every old value is requested up front, next to the row's inputs -- the row is a chain of
    // ~20 scattered accesses, and the read-modify-writes behind the chain rule's ~600 instructions were fully exposed
    float old_m[3] = {0.f, 0.f, 0.f}, old_s[3] = {0.f, 0.f, 0.f}, old_c[3] = {0.f, 0.f, 0.f}, old_o = 0.f;
    float4 old_q = {0.f, 0.f, 0.f, 0.f};
    float4 sr0 = {0.f, 0.f, 0.f, 0.f}, sr1 = sr0, sr2 = sr0, sr3 = sr0;
    float4* const srow = SINKROWS ? reinterpret_cast<float4*>(g_means3d) + 4 * (size_t)i : nullptr;
    if (SINKROWS) {
      sr0 = srow[0]; sr1 = srow[1]; sr2 = srow[2]; sr3 = srow[3];
    } else if (ACCUMULATE) {
#pragma unroll
      for (int k = 0; k < 3; k++) old_m[k] = g_means3d[3 * (size_t)i + k];
      if (!COV) {
#pragma unroll
        for (int k = 0; k < 3; k++) old_s[k] = g_scales[3 * (size_t)i + k];
        old_q = reinterpret_cast<const float4*>(g_rots)[i];
      }
      if (AOS) {
        old_o = o_opac[i];
#pragma unroll
        for (int k = 0; k < 3; k++) old_c[k] = o_col[3 * (size_t)i + k];
      }
    }
    if (AOS) {
      const float4 a0 = rows[4 * (size_t)i], a1 = rows[4 * (size_t)i + 1];
      const float cb = reinterpret_cast<const float*>(rows + 4 * (size_t)i + 2)[0];
      if (AUXO) {   // slots 9..11: dL/daux_colors of a reverse walk with aux channels (fresh gradients only)
        const float* const ar = reinterpret_cast<const float*>(rows + 4 * (size_t)i + 2);
        o_aux[3 * (size_t)i + 0] = ar[1]; o_aux[3 * (size_t)i + 1] = ar[2]; o_aux[3 * (size_t)i + 2] = ar[3];
        const float4 a3 = rows[4 * (size_t)i + 3];   // slots 12..14: the aux image's dL/dconic (below)
        gA2 = a3.x; gB2 = a3.y; gC2 = a3.z;
      }
      if (ABSO) {   // slots 9, 10: the absolute sums of a reverse walk with ABS (fresh gradients only); column 2 as dL/dmeans2D's
        const float* const ar = reinterpret_cast<const float*>(rows + 4 * (size_t)i + 2);
        o_abs[3 * (size_t)i + 0] = ar[1]; o_abs[3 * (size_t)i + 1] = ar[2]; o_abs[3 * (size_t)i + 2] = 0.f;
      }
      gnx = a0.x; gny = a0.y; gA = a0.z; gB = a0.w; gC = a1.x;
      if (staged) {   // the workgroup's slice of dL/dmeans2D sits in LDS and leaves as whole lines (lr_project_bwd_kernel)
        float* const o = m2d_slice + 3 * (i - slice_base);
        o[0] = gnx; o[1] = gny; o[2] = 0.f;
      } else {
        o_mean2d[3 * (size_t)i + 0] = gnx; o_mean2d[3 * (size_t)i + 1] = gny; o_mean2d[3 * (size_t)i + 2] = 0.f;
      }
      if (SINKROWS) {
        sr2.z += a1.y; sr2.w += a1.z; sr3.x += a1.w; sr3.y += cb;   // slots 10 opacity, 11-13 colour
      } else {
        o_opac[i] = old_o + a1.y;
        o_col[3 * (size_t)i + 0] = old_c[0] + a1.z; o_col[3 * (size_t)i + 1] = old_c[1] + a1.w; o_col[3 * (size_t)i + 2] = old_c[2] + cb;
      }
    } else {
      gnx = g_mean2d[3 * (size_t)i]; gny = g_mean2d[3 * (size_t)i + 1];
      const float4 gc4 = reinterpret_cast<const float4*>(g_conic)[i];
      gA = gc4.x; gB = gc4.y; gC = gc4.z;
    }
    lr_project_bwd_row<ACCUMULATE, COV>(v, i, means, scales, rots, gnx, gny, gA, gB, gC, gm, gs, gq);
    if (AUXO) {
      // The aux image's dL/dconic goes through the chain rule on its own and the results are added -- the arithmetic of two
      // rasterizer calls.  (The conic part is ill-conditioned in fp32 for needle-shaped Gaussians: one evaluation on the
      // summed dL/dconic differs from two evaluations added by as much as either differs from the exact value.  The centre
      // part, dL/dmean, is not: it arrives as one sum.)
      float gm2[3], gs2[3] = {0.f, 0.f, 0.f}, gq2[4] = {0.f, 0.f, 0.f, 0.f};
      lr_project_bwd_row<ACCUMULATE, COV>(v, i, means, scales, rots, 0.f, 0.f, gA2, gB2, gC2, gm2, gs2, gq2);
#pragma unroll
      for (int k = 0; k < 3; k++) { gm[k] += gm2[k]; gs[k] += gs2[k]; }
#pragma unroll
      for (int k = 0; k < 4; k++) gq[k] += gq2[k];
    }
    if (SINKROWS) {    // running sums over views, one row per Gaussian
      sr0.x += gm[0]; sr0.y += gm[1]; sr0.z += gm[2]; sr0.w += gs[0];
      sr1.x += gs[1]; sr1.y += gs[2]; sr1.z += gq[0]; sr1.w += gq[1];
      sr2.x += gq[2]; sr2.y += gq[3];
      srow[0] = sr0; srow[1] = sr1; srow[2] = sr2; srow[3] = sr3;
    } else if (ACCUMULATE) {  // running sums over views (log_amd.dist)
#pragma unroll
      for (int k = 0; k < 3; k++) g_means3d[3 * (size_t)i + k] = old_m[k] + gm[k];
      if (!COV) {
#pragma unroll
        for (int k = 0; k < 3; k++) g_scales[3 * (size_t)i + k] = old_s[k] + gs[k];
        reinterpret_cast<float4*>(g_rots)[i] = float4{old_q.x + gq[0], old_q.y + gq[1], old_q.z + gq[2], old_q.w + gq[3]};
      }
    } else {
      g_means3d[3 * (size_t)i + 0] = gm[0]; g_means3d[3 * (size_t)i + 1] = gm[1]; g_means3d[3 * (size_t)i + 2] = gm[2];
      if (!COV) {
        g_scales[3 * (size_t)i + 0] = gs[0]; g_scales[3 * (size_t)i + 1] = gs[1]; g_scales[3 * (size_t)i + 2] = gs[2];
        reinterpret_cast<float4*>(g_rots)[i] = float4{gq[0], gq[1], gq[2], gq[3]};
      }
    }
    if (CAM) {
      // behind the row's stores and behind a scheduling fence: interleaved with the fp32 chain the double chain took every
      // register a wave can have (256 VGPRs + AGPRs, one wave per SIMD); the row's 40 input bytes are read again (cache hits)
      __builtin_amdgcn_sched_barrier(0);
      const float pf[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
      const float sf[3] = {scales[3 * i] * v.scale_modifier, scales[3 * i + 1] * v.scale_modifier, scales[3 * i + 2] * v.scale_modifier};
      const float4 q4 = reinterpret_cast<const float4*>(rots)[i];
      const float qf[4] = {q4.x, q4.y, q4.z, q4.w};
      lr_camera_row(v, pf, sf, qf, gnx, gny, gA, gB, gC, cam);
    }
}

// One workgroup owns LR_PBWD_ROWS consecutive Gaussians.  Their live flags are read coalesced; the live rows are
// COMPACTED into an LDS list and the chain rule (~600 VALU instructions per row) then runs on full waves: with 15 % of
// the rows live (30 M Gaussians, opacity 0.999) every wave of a one-thread-per-Gaussian kernel still met a live lane and
// ran all of it at 15 % lane occupancy (VALU busy 71 % of the launch).
#define LR_PBWD_ROWS 1024
// AOS (lograst_backward): the reverse walk's nine sums of a Gaussian sit in ONE 64-byte row of `rows` (slots: 0-1 mean
// x y, 2-4 conic A B C, 5 opacity, 6-8 colour r g b: include/lograst.h LOGRAST_BWD_ROW_FLOATS) -- a memory-side atomic
// costs one operation per 64-byte LINE whatever the number of lanes in it (tools/micro/atomic_lines.hip: 17-21 G lines/s
// chip-wide for 1, 9 or 16 lanes per line), so the reverse walk commits a (wave, Gaussian) visit with one line operation
// instead of four.  This kernel then also hands out the API's separate outputs: dL/dmeans2D (written for every row: it
// is a per-view output), dL/dopacity and dL/dcolour (written, or added to the running sums when ACCUMULATE).
// !AOS (lograst_project_backward, the isolated chain rule): g_mean2d [n, 3] / g_conic [n, 4] in, as before.
// SINKROWS (lograst_backward with LOGRAST_BWD_ACCUMULATE_ROWS; implies ACCUMULATE and AOS, not COV): the caller's running
// sums are ONE 64-byte row per Gaussian too (`g_means3d` = [N][16]: slots 0-2 dL/dmeans3D, 3-5 dL/dscales, 6-9
// dL/drotations, 10 dL/dopacity, 11-13 dL/dcolour, 14-15 untouched) -- a live Gaussian then costs one read-modify-write of
// one line instead of five in five arrays (the live rows are scattered: at 30 M Gaussians 7 % of them, each piece of 4-16
// bytes pulling its own 64-byte line through the memory system in both directions).
// AUXO (lograst_backward_aux; AOS, fresh gradients, not COV): the rows' slots 9..11 leave as dL/daux_colors [N, 3] -- a
// live row's values, zeros for the others, exactly as dL/dcolour -- and slots 12..14 hold the aux image's dL/dconic, which
// takes its own pass through the chain rule inside the same launch (lr_pbwd_live_row).
// CAM (lograst_backward_camera / lograst_project_backward_camera; fresh gradients, not COV, not AUXO): every live row's
// terms of dL/dviewmatrix and dL/dprojmatrix -- LR_CAM_SUMS sums, the terms from a second, double pass over the row
// (lr_camera_row) -- are added up per lane, per wave (shuffles), per workgroup (LDS, wave order), and the workgroup STORES its partials to row
// blockIdx.x of cam_out [workgroups, LR_CAM_SUMS]: a workgroup without a live row stores zeros, lanes without a row add
// zeros.  No atomics: every workgroup adding into the same two lines is the worst shape for a float atomic, and the order of
// the additions would change from run to run.  lr_camera_finish_kernel adds the rows up in workgroup order.
// ABSO (lograst_backward_abs; AOS, fresh gradients, not COV, not AUXO, not CAM): the rows' slots 9 and 10 -- the reverse
// walk's sums of |per-pixel term of dL/dmean x, y| -- leave as dl_dmeans2d_abs [N, 3] (column 2 = 0): a live row's values,
// zeros for the others through the block-wide clear, exactly as dL/dcolour.  Plain 12-byte stores like dL/dmeans2D's in this
// form: the staged slice (STAGE) exists for running sums only, which this output does not come with.
// WAVES: waves per SIMD the register allocator aims for (1 = its own choice: ~130 VGPRs, three waves).  Measured, 30 M
// Gaussians, running sums / fresh gradients: default 374 / 736 us, 4 waves (128 VGPRs, no scratch) 391 / 865, 5 (spills)
// 473 / 877, 6: 518 / 918 -- more resident workgroups make the scattered rows' traffic worse, not better.  A band view
// (nearly all flag pass: a fraction of a percent of 100 M rows is live) gains from four: 738 -> 638 us -- the row-major
// sink's kernel exists in both forms and band views launch the second (unless they take the compact-list form below, the
// default; the current compiler spills 10 VGPRs in it, 22 before the staged slice: profiles/chain_rule_dmeans2d_lines.md).
template <bool ACCUMULATE, bool TOUCHED, bool COV, bool AOS, bool SINKROWS = false, int WAVES = 1, bool AUXO = false,
          bool CAM = false, bool ABSO = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES)))
lr_project_bwd_kernel(LrView v, int N, const float* __restrict__ means, const float* __restrict__ scales,
                      const float* __restrict__ rots, const int* __restrict__ radii,
                      const float* __restrict__ g_mean2d, const float* __restrict__ g_conic,
                      const float4* __restrict__ rows, float* __restrict__ o_mean2d, float* __restrict__ o_opac,
                      float* __restrict__ o_col,
                      const float* __restrict__ pw, float* __restrict__ g_means3d, float* __restrict__ g_scales,
                      float* __restrict__ g_rots, int clear_inside, float* __restrict__ o_aux = nullptr,
                      float* __restrict__ cam_out = nullptr, float* __restrict__ o_abs = nullptr) {
  static_assert(!ABSO || (AOS && !ACCUMULATE && !COV && !SINKROWS && !AUXO && !CAM), "absolute sums: fresh gradients from the accumulator rows only, no aux, no camera sums");
  static_assert(!CAM || (!ACCUMULATE && !COV && !SINKROWS && !AUXO), "camera sums: fresh gradients, scales / rotations, no aux");
  static_assert(!AUXO || (AOS && !ACCUMULATE && !COV && !SINKROWS), "dL/daux_colors: fresh gradients from the accumulator rows only");
  __shared__ uint32_t live_list[LR_PBWD_ROWS];
  __shared__ uint32_t live_count;
  __shared__ uint32_t cam_count[CAM ? LR_PBWD_ROWS / 64 : 1];   // (CAM: live rows per (round, wave) slice of the block)
  // STAGE (the instantiations the large-input running-sum route launches; taken when clear_inside == 0): the workgroup's
  // slice of dL/dmeans2D -- 1024 rows x 12 bytes = 12 288 contiguous bytes, a multiple of 64 -- is built in LDS (zeros,
  // then the live rows' values) and leaves with 16-byte stores that cover whole 64-byte lines.  The memory side charges
  // write transactions, a partial line as much as a full one: before, lr_zero_floats_kernel streamed the array's zeros in a
  // launch of its own and every live row then re-opened one or two of those lines with a 12-byte store.  Measured, 30 M rows
  // (profiles/chain_rule_dmeans2d_lines.md): the kernel itself 344 -> 352 us WITH the array's 360 MB, the 66 us zero pass
  // gone (the stage 432 -> 356 us; opacity = rand 642 -> 507); scattered write requests per live row 1.80 -> 0.92.  LDS per
  // workgroup 4 -> 16 KB (nine workgroups per CU by LDS, three by registers).  Handing the row's values out behind the chain
  // rule instead of in front of it (no store between the row's gathers) cost 8 more VGPRs and 7-10 us: not kept.
  constexpr bool STAGE = AOS && ACCUMULATE;
  __shared__ __attribute__((aligned(16))) float m2d_slice[STAGE ? 3 * LR_PBWD_ROWS : 4];
  const bool staged = STAGE && !clear_inside;
  const int tid = threadIdx.x, base = blockIdx.x * LR_PBWD_ROWS;
  if (tid == 0) live_count = 0u;
  // the live flags of the workgroup's rows, requested before anything else and all at once: most workgroups hold no live
  // row at all, and their whole life was clear -> barrier -> radii -> (radii > 0 ?) point_weight -> barrier, one memory
  // round trip after the other (30 M Gaussians: 0.21 of the kernel's 0.43 ms with not a single live row)
  int rad_k[LR_PBWD_ROWS / 256];
  float pw_k[LR_PBWD_ROWS / 256];
#pragma unroll
  for (int k = 0; k < LR_PBWD_ROWS / 256; k++) {
    const int i = base + k * 256 + tid;
    // (TOUCHED: the forward cleared point_weight for every row and only composited Gaussians -- radii > 0 -- ever raised
    // it: the blend weight alone is the live flag, radii is not read: 0.4 of the 2.0 GB a 100 M-row band view streams)
    rad_k[k] = TOUCHED ? 1 : (i < N ? radii[i] : 0);
    pw_k[k] = (TOUCHED && i < N) ? pw[i] : 1.f;
  }
  typedef float lr_f4v __attribute__((ext_vector_type(4)));
  if (staged) {   // zeros for the whole slice, in LDS, while the flag loads are in flight (three 16-byte LDS stores per thread)
#pragma unroll
    for (int k = 0; k < 3 * LR_PBWD_ROWS / 4 / 256; k++)
      reinterpret_cast<lr_f4v*>(m2d_slice)[k * 256 + tid] = lr_f4v{0.f, 0.f, 0.f, 0.f};
  }
  if (AOS && clear_inside) {
    // the per-view / per-call outputs are defined for every row: the block's whole slice is cleared with full-width
    // stores first (row-by-row 12-byte stores from the flag pass below cost the 30 M view 0.2 ms), the live rows
    // overwrite theirs after the barrier.  (Large inputs with running sums take the staged form above instead.)
    const int rows_here = min(LR_PBWD_ROWS, N - base);
    // (a scalar head up to the first 16-byte boundary, then full-width stores, then a scalar tail: the C ABI asks only
    // for 4-byte alignment of these outputs -- round-4 advisory; torch's allocations always take the head-less path)
    auto clear = [&](float* p0, int floats) {
      const int head = min(floats, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p0) & 15u)) & 15u) >> 2));
      if (tid < head) p0[tid] = 0.f;
      float* p = p0 + head;
      floats -= head;
      const int n4 = floats >> 2;
      lr_f4v* q = reinterpret_cast<lr_f4v*>(p);
      for (int t = tid; t < n4; t += 256) q[t] = lr_f4v{0.f, 0.f, 0.f, 0.f};
      for (int t = (n4 << 2) + tid; t < floats; t += 256) p[t] = 0.f;
    };
    if (rows_here > 0) {
      clear(o_mean2d + 3 * (size_t)base, 3 * rows_here);
      if (!ACCUMULATE && !SINKROWS) {
        // fresh gradients (the autograd route: what unmodified LoG gets): every output is defined for every row -- the
        // whole slice of each array with full-width stores here, instead of 12-byte pieces per dead row from the flag
        // pass below (three store instructions covering a third of every line each)
        clear(o_opac + (size_t)base, rows_here); clear(o_col + 3 * (size_t)base, 3 * rows_here);
        if (AUXO) clear(o_aux + 3 * (size_t)base, 3 * rows_here);
        if (ABSO) clear(o_abs + 3 * (size_t)base, 3 * rows_here);
        clear(g_means3d + 3 * (size_t)base, 3 * rows_here);
        if (COV) {
          clear(v.g_cov3d + 6 * (size_t)base, 6 * rows_here);
        } else {
          clear(g_scales + 3 * (size_t)base, 3 * rows_here);
          clear(g_rots + 4 * (size_t)base, 4 * rows_here);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LR_PBWD_ROWS / 256; k++) {
    const int i = base + k * 256 + tid;
    const bool live = i < N && rad_k[k] > 0 && (!TOUCHED || pw_k[k] > 0.f);
    if (!ACCUMULATE && !AOS && i < N && !live) {   // isolated chain rule: culled / untouched rows get zero gradients (AOS: cleared above)
      g_means3d[3 * (size_t)i + 0] = 0.f; g_means3d[3 * (size_t)i + 1] = 0.f; g_means3d[3 * (size_t)i + 2] = 0.f;
      if (COV) {
#pragma unroll
        for (int c = 0; c < 6; c++) v.g_cov3d[6 * (size_t)i + c] = 0.f;
      } else {
        g_scales[3 * (size_t)i + 0] = 0.f; g_scales[3 * (size_t)i + 1] = 0.f; g_scales[3 * (size_t)i + 2] = 0.f;
        reinterpret_cast<float4*>(g_rots)[i] = float4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const uint64_t m = __ballot(live);
    if (CAM) {   // (the list is built below, in row order)
      if ((tid & 63) == 0) cam_count[k * 4 + (tid >> 6)] = (uint32_t)__popcll(m);
    } else if (m) {
      uint32_t first = 0;
      if ((tid & 63) == 0) first = atomicAdd(&live_count, (uint32_t)__popcll(m));
      first = (uint32_t)__shfl((int)first, 0);
      if (live) live_list[first + (uint32_t)__popcll(m & ((1ull << (tid & 63)) - 1ull))] = (uint32_t)i;
    }
  }
  __syncthreads();
  if (CAM) {
    // The order in which the waves' atomics reserve their slots changes from run to run, and with it which lane adds which
    // row's terms: the camera sums would differ in their last bits.  Here every (round, wave) slice of the list starts
    // behind the slices in front of it: the list is in row order, and identical inputs give identical sums.
#pragma unroll
    for (int k = 0; k < LR_PBWD_ROWS / 256; k++) {
      const int i = base + k * 256 + tid;
      const bool live = i < N && rad_k[k] > 0 && (!TOUCHED || pw_k[k] > 0.f);
      const uint64_t m = __ballot(live);
      uint32_t first = 0;
      for (int w = 0; w < k * 4 + (tid >> 6); w++) first += cam_count[w];
      if (live) live_list[first + (uint32_t)__popcll(m & ((1ull << (tid & 63)) - 1ull))] = (uint32_t)i;
    }
    if (tid == 0) {
      uint32_t total = 0;
      for (int w = 0; w < LR_PBWD_ROWS / 64; w++) total += cam_count[w];
      live_count = total;
    }
    __syncthreads();
  }
  const uint32_t n = live_count;
  float cam[CAM ? LR_CAM_SUMS : 1];
  if (CAM) {
#pragma unroll
    for (int c = 0; c < LR_CAM_SUMS; c++) cam[c] = 0.f;
  }
  for (uint32_t j = (uint32_t)tid; j < n; j += 256u)
    lr_pbwd_live_row<ACCUMULATE, COV, AOS, SINKROWS, AUXO, CAM, ABSO>(v, (int)live_list[j], means, scales, rots, g_mean2d, g_conic, rows,
                                                                      o_mean2d, o_opac, o_col, g_means3d, g_scales, g_rots,
                                                                      STAGE ? m2d_slice : nullptr, base, staged, o_aux, cam, o_abs);
  if (CAM && n == 0u) {   // (most workgroups of a large view: no live row, nothing to reduce)
    if (tid < LR_CAM_SUMS) cam_out[(size_t)blockIdx.x * LR_CAM_SUMS + tid] = 0.f;
  } else if (CAM) {
    // lane -> wave (a butterfly: every lane ends with the wave's sum, in an order fixed by the lane numbers) -> workgroup
    __shared__ float cam_wave[256 / 64][LR_CAM_SUMS];
#pragma unroll
    for (int c = 0; c < LR_CAM_SUMS; c++) {
      float x = cam[c];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
      cam[c] = x;
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int c = 0; c < LR_CAM_SUMS; c++) cam_wave[tid >> 6][c] = cam[c];
    }
    __syncthreads();
    if (tid < LR_CAM_SUMS)
      cam_out[(size_t)blockIdx.x * LR_CAM_SUMS + tid] = ((cam_wave[0][tid] + cam_wave[1][tid]) + cam_wave[2][tid]) + cam_wave[3][tid];
  }
  if (staged) {
    // the slice leaves: every row of the block is defined here (zero unless live), 16 bytes per lane and 1 KB per wave and
    // store instruction -- whole lines (three instructions for a full block); non-temporal like the zero pass it replaces
    // (360 MB per 30 M-row view that nothing reads back soon).  The C ABI asks only for 4-byte alignment: then a scalar head
    // up to the first 16-byte boundary and a scalar tail (the LDS side of the middle part reads four floats one by one);
    // torch's allocations take the head-less path.
    __syncthreads();
    const int rows_here = min(LR_PBWD_ROWS, N - base);
    float* const p0 = o_mean2d + 3 * (size_t)base;
    int floats = 3 * rows_here;
    const int head = min(floats, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p0) & 15u)) & 15u) >> 2));
    if (tid < head) p0[tid] = m2d_slice[tid];
    floats -= head;
    const int n4 = floats >> 2;
    lr_f4v* const q = reinterpret_cast<lr_f4v*>(p0 + head);
    if (head == 0) {
      for (int t = tid; t < n4; t += 256) __builtin_nontemporal_store(reinterpret_cast<const lr_f4v*>(m2d_slice)[t], q + t);
    } else {
      for (int t = tid; t < n4; t += 256) {
        const float* const l = m2d_slice + head + 4 * t;
        __builtin_nontemporal_store(lr_f4v{l[0], l[1], l[2], l[3]}, q + t);
      }
    }
    for (int t = (n4 << 2) + tid; t < floats; t += 256) p0[head + t] = m2d_slice[head + t];
  }
}


// ---- the chain rule over a COMPACT list of the live rows (round 5) ---------------------------------------------------------
// On large inputs whose gradients are running sums (nothing is written for a dead row) the kernel above spends half its
// time deciding that rows are dead: 29 K workgroups of a 30 M-row view, each a chain of flag load -> barrier -> (no live
// row) at three resident workgroups per CU (its chain rule needs ~130 VGPRs) -- 0.21 of its 0.40 ms; a band view of 100 M
// rows 0.5 of its 0.74.  So the decision gets a kernel of its own, shaped like a copy: `lr_pbwd_compact_kernel` streams
// point_weight (16 bytes per lane, low registers, full occupancy) and appends the indices of the rows with weight > 0 to a
// list, one slot-reserving atomic per 8192 rows; `lr_pbwd_list_kernel` then runs the chain rule over that list with a
// fixed grid (the count never travels to the host) and every lane busy.  The list needs no buffer of its own: slots 12-15
// of the reverse walk's 64-byte accumulator rows are unused (LOGRAST_BWD_ROW_FLOATS: nine sums per row), so entry j sits
// in row 1 + j / 4, slot 12 + j % 4, and the count in row 0, slot 12 (cleared by lr_zero_words_kernel before the pass).
// Same per-row code (lr_pbwd_live_row), so the same gradients bit for bit.
#define LR_PBWD_CHUNK 8192             // rows per workgroup of the compaction pass (one atomic each; 32 KB of LDS for a chunk that is all live)
LR_DEV uint32_t* lr_pbwd_list_slot(float4* rows, uint32_t j) {
  return reinterpret_cast<uint32_t*>(rows + 4 * (size_t)(1u + (j >> 2)) + 3) + (j & 3u);
}
__global__ void __launch_bounds__(1024)
lr_pbwd_compact_kernel(const float* __restrict__ pw, int N, float4* __restrict__ rows) {
  __shared__ uint32_t live[LR_PBWD_CHUNK];                    // worst case: every row of the chunk is live
  __shared__ uint32_t cnt, base_s;
  const int tid = threadIdx.x;
  const int base = blockIdx.x * LR_PBWD_CHUNK;
  if (tid == 0) cnt = 0u;
  __syncthreads();
  typedef float lr_f4v __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int k = 0; k < LR_PBWD_CHUNK / 4096; k++) {           // four rows per lane and round, all rounds requested up front
    const int i0 = base + (k * 1024 + tid) * 4;
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (i0 + 3 < N && ((reinterpret_cast<uintptr_t>(pw) & 15u) == 0u)) {
      const lr_f4v q = __builtin_nontemporal_load(reinterpret_cast<const lr_f4v*>(pw + i0));
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; u++) w[u] = (i0 + u < N) ? pw[i0 + u] : 0.f;
    }
    const int n_live = (w[0] > 0.f) + (w[1] > 0.f) + (w[2] > 0.f) + (w[3] > 0.f);
    // position inside the chunk's list: wave prefix over the lanes' counts, one LDS atomic per wave
    int inc = n_live;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d);
      if ((tid & 63) >= d) inc += up;
    }
    uint32_t first = 0;
    const int total = __shfl(inc, 63);
    if ((tid & 63) == 63 && total) first = atomicAdd(&cnt, (uint32_t)total);
    first = (uint32_t)__shfl((int)first, 63);
    uint32_t pos = first + (uint32_t)(inc - n_live);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (w[u] > 0.f) live[pos++] = (uint32_t)(i0 + u);
  }
  __syncthreads();
  const uint32_t n = cnt;
  if (tid == 0) base_s = n ? atomicAdd(reinterpret_cast<uint32_t*>(rows + 3), n) : 0u;   // row 0, slot 12: the list's length
  __syncthreads();
  const uint32_t b = base_s;
  for (uint32_t j = (uint32_t)tid; j < n; j += 1024u) *lr_pbwd_list_slot(rows, b + j) = live[j];
}

template <bool ACCUMULATE, bool SINKROWS>
__global__ void __launch_bounds__(256)
lr_pbwd_list_kernel(LrView v, int N, const float* __restrict__ means, const float* __restrict__ scales,
                    const float* __restrict__ rots, float4* __restrict__ rows, float* __restrict__ o_mean2d,
                    float* __restrict__ o_opac, float* __restrict__ o_col, float* __restrict__ g_means3d,
                    float* __restrict__ g_scales, float* __restrict__ g_rots) {
  const uint32_t n = min(reinterpret_cast<const uint32_t*>(rows + 3)[0], (uint32_t)N);
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
    const uint32_t i = *lr_pbwd_list_slot(rows, j);
    if (i < (uint32_t)N)
      lr_pbwd_live_row<ACCUMULATE, false, true, SINKROWS>(v, (int)i, means, scales, rots, nullptr, nullptr, rows, o_mean2d,
                                                          o_opac, o_col, g_means3d, g_scales, g_rots);
  }
}

// ---- camera gradients: the workgroups' partial sums -> dL/dviewmatrix, dL/dprojmatrix ----------------------------------
// partials [G, LR_CAM_SUMS] as lr_project_bwd_kernel<CAM> stored them: slots 3 r + k (r = 0..3, k = 0..2) dL/dV[r][k], slots
// 12 + 3 r + c' dL/dP[r][c] with c' = 0, 1, 2 for the columns c = 0, 1, 3.  Everything is added in workgroup order, in double,
// with a bracketing that depends on G alone -- identical inputs give identical bits -- and rounded to fp32 once: block b of
// B takes the rows [b chunk, (b + 1) chunk); in it LR_CAM_GROUPS lane groups of LR_CAM_SUMS lanes take consecutive sub-ranges,
// and their sums are added in group order.  B = 1 (G <= LR_CAM_ONE_BLOCK rows, views of up to 2 M Gaussians): that block
// writes dV [4, 4] and dP [4, 4] itself -- whole, column 3 of dV and column 2 of dP are 0.  Otherwise the blocks leave their
// sums as doubles in `stage` [B, LR_CAM_SUMS] and lr_camera_total_kernel adds those in block order.  (One block for the 29 297
// rows of a 30 M-Gaussian view took 0.22 ms, as much as the camera sums cost the chain-rule launch itself.)
#define LR_CAM_GROUPS 42        // 42 x 24 = 1008 of 1024 lanes
#define LR_CAM_ONE_BLOCK 2048
#define LR_CAM_BLOCKS 64
LR_DEV void lr_camera_write(const double* sums, int tid, float* __restrict__ dV, float* __restrict__ dP) {   // tid < 32
  const int mat = tid >> 4, r = (tid >> 2) & 3, col = tid & 3;
  const bool zero = mat ? col == 2 : col == 3;
  const int slot = mat ? 12 + 3 * r + (col == 3 ? 2 : col) : 3 * r + col;
  (mat ? dP : dV)[4 * r + col] = zero ? 0.f : (float)sums[slot];
}
__global__ void __launch_bounds__(1024)
lr_camera_finish_kernel(const float* __restrict__ partials, int G, double* __restrict__ stage, float* __restrict__ dV,
                        float* __restrict__ dP) {
  __shared__ double part[LR_CAM_GROUPS][LR_CAM_SUMS];
  __shared__ double sums[LR_CAM_SUMS];
  const int tid = threadIdx.x, g = tid / LR_CAM_SUMS, c = tid - g * LR_CAM_SUMS;
  const int chunk = (G + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = min(G, (int)blockIdx.x * chunk), r1 = min(G, r0 + chunk);
  if (g < LR_CAM_GROUPS) {
    const int sub = (r1 - r0 + LR_CAM_GROUPS - 1) / LR_CAM_GROUPS;
    const int w0 = min(r1, r0 + g * sub), w1 = min(r1, w0 + sub);
    double acc = 0.0;
#pragma unroll 8
    for (int w = w0; w < w1; w++) acc += (double)partials[(size_t)w * LR_CAM_SUMS + c];
    part[g][c] = acc;
  }
  __syncthreads();
  if (tid < LR_CAM_SUMS) {
    double acc = 0.0;
    for (int k = 0; k < LR_CAM_GROUPS; k++) acc += part[k][tid];
    if (gridDim.x == 1) sums[tid] = acc; else stage[(size_t)blockIdx.x * LR_CAM_SUMS + tid] = acc;
  }
  if (gridDim.x == 1) {
    __syncthreads();
    if (tid < 32) lr_camera_write(sums, tid, dV, dP);
  }
}
__global__ void __launch_bounds__(64)
lr_camera_total_kernel(const double* __restrict__ stage, int B, float* __restrict__ dV, float* __restrict__ dP) {
  __shared__ double sums[LR_CAM_SUMS];
  const int tid = threadIdx.x;
  if (tid < LR_CAM_SUMS) {
    double acc = 0.0;
    for (int b = 0; b < B; b++) acc += stage[(size_t)b * LR_CAM_SUMS + tid];
    sums[tid] = acc;
  }
  __syncthreads();
  if (tid < 32) lr_camera_write(sums, tid, dV, dP);
}
// the partials' rows, then (8-byte aligned: a row is 96 bytes) the blocks' double sums
static size_t lr_camera_rows(int N) { return (size_t)(N > 0 ? (N + LR_PBWD_ROWS - 1) / LR_PBWD_ROWS : 1); }
size_t lr_camera_scratch_bytes(int N) {
  return sizeof(float) * LR_CAM_SUMS * lr_camera_rows(N) + sizeof(double) * LR_CAM_SUMS * LR_CAM_BLOCKS;
}
static void lr_launch_camera_finish(float* partials, int N, float* dV, float* dP, hipStream_t s) {
  const int G = (int)lr_camera_rows(N);
  double* stage = reinterpret_cast<double*>(partials + (size_t)G * LR_CAM_SUMS);
  const int B = G <= LR_CAM_ONE_BLOCK ? 1 : LR_CAM_BLOCKS;
  hipLaunchKernelGGL(lr_camera_finish_kernel, dim3(B), dim3(1024), 0, s, partials, G, stage, dV, dP);
  if (B > 1) hipLaunchKernelGGL(lr_camera_total_kernel, dim3(1), dim3(64), 0, s, stage, B, dV, dP);
}

void lr_launch_project_bwd(const LrView& v, const LrProjectBwdArgs& a, hipStream_t s) {
  const int N = a.N;
  if (N <= 0) return;
  // What the call is, in one place.  The extras' entry points checked: fresh gradients, no cov3d_precomp, whole image, one
  // extra at a time (aux and abs: rows), so every output is cleared inside for them.
  const bool touched = a.pw != nullptr, aos = a.rows != nullptr, cov = v.cov3d != nullptr;
  const bool cam = a.cam_partials != nullptr, auxo = a.o_aux != nullptr, abso = a.o_abs != nullptr;
  const bool band_view = v.ty0 > 0 || v.ty1 < v.gy;
  // dL/dmeans2D is a per-view output, defined for every row.  When the other gradients are running sums (nothing else is
  // written for a dead row) and the input is large (clear_inside == 0), the kernel's workgroups neither clear their slice
  // between their flag reads and their barrier nor overwrite live rows with 12-byte stores: the slice is staged in LDS and
  // leaves as whole lines (lr_project_bwd_kernel: STAGE) -- no zero pass in front of the kernel.  Only the compact-list
  // form below, which has no per-block slice, still has lr_zero_floats_kernel stream the zeros first (non-temporal 16-byte
  // stores; a band view of 100 M rows 1040 -> 730 us against clearing inside, with the radii read gone).  With fresh
  // gradients (every output zeroed for every dead row: 68 bytes per row) a separate zero pass LOSES (30 M: 763 -> 858 us):
  // cleared inside.
  const int clear_inside = (aos && (a.accumulate || a.sink_rows) && a.big_input) ? 0 : 1;
  // Large inputs, running sums, the forward's point_weight at hand, no cov3d_precomp: the live rows through a compact list
  // (see lr_pbwd_compact_kernel) -- on BAND views, where a per cent of the rows is live and the one-kernel form is nearly
  // all flag pass (100 M rows, band 3 of 8: 929 -> 490 us).  On full views the chain rule is bound by its scattered lines
  // either way (~7 lines per live row at ~50 G lines/s): measured at 30 M rows, list / one kernel: 7 % live 419 / 469 us,
  // 7.5 % (trained-like) 451 / 481, 14 % (opacity = rand) 690 / 610 -- not worth a second form there.
  // LOGRAST_PBWD_LIST: 0 never, 1 band views (default), 2 always.
  const int list_knob = lr_knob(LRKNOB_PBWD_LIST);
  const bool list = (list_knob == 2 || (list_knob == 1 && band_view)) && !clear_inside && touched && !cov && N >= 8;
  // The one-kernel form's choice; template arguments <ACCUMULATE, TOUCHED, COV, AOS, SINKROWS, WAVES, AUXO, CAM, ABSO>.  (The
  // tables name the kernels in the order in which they have always been instantiated, "true" first: that is the order of the
  // device code, which tools/device_asm_digest.py holds still.  So an entry's index is [!flag].)
#define LR_K(...) lr_project_bwd_kernel<__VA_ARGS__>
  typedef decltype(&LR_K(false, true, false, true, false, 3, false, true)) Kernel;
  static constexpr Kernel cam_kernel[2][2] = {   // [!aos][!touched]
      {LR_K(false, true, false, true, false, 3, false, true), LR_K(false, false, false, true, false, 3, false, true)},
      {LR_K(false, true, false, false, false, 3, false, true), LR_K(false, false, false, false, false, 3, false, true)}};
  static constexpr Kernel aux_kernel[2] = {LR_K(false, true, false, true, false, 1, true),   // [!touched]
                                           LR_K(false, false, false, true, false, 1, true)};
  static constexpr Kernel abs_kernel[2] = {LR_K(false, true, false, true, false, 1, false, false, true),   // [!touched]
                                           LR_K(false, false, false, true, false, 1, false, false, true)};
  static constexpr decltype(&lr_pbwd_list_kernel<true, true>) list_kernel[2] = {lr_pbwd_list_kernel<true, true>,   // [!sink_rows]
                                                                                   lr_pbwd_list_kernel<true, false>};
  static constexpr Kernel sink_kernel[3] = {LR_K(true, true, false, true, true, 4),   // [0] touched, band view: the four-wave form (WAVES, above)
                                            LR_K(true, true, false, true, true),      // [1] touched, whole view
                                            LR_K(true, false, false, true, true)};    // [2] no point_weight
  static constexpr Kernel plain_kernel[2][2][2][2] = {   // [!accumulate][!touched][!cov][!aos]
      {{{LR_K(true, true, true, true), LR_K(true, true, true, false)}, {LR_K(true, true, false, true), LR_K(true, true, false, false)}},
       {{LR_K(true, false, true, true), LR_K(true, false, true, false)}, {LR_K(true, false, false, true), LR_K(true, false, false, false)}}},
      {{{LR_K(false, true, true, true), LR_K(false, true, true, false)}, {LR_K(false, true, false, true), LR_K(false, true, false, false)}},
       {{LR_K(false, false, true, true), LR_K(false, false, true, false)}, {LR_K(false, false, false, true), LR_K(false, false, false, false)}}}};
#undef LR_K
  const Kernel kernel = cam ? cam_kernel[!aos][!touched] : auxo ? aux_kernel[!touched] : abso ? abs_kernel[!touched]
                        : a.sink_rows ? sink_kernel[!touched ? 2 : band_view ? 0 : 1]   // (lograst_backward checked: rows != NULL, no cov3d)
                                      : plain_kernel[!a.accumulate][!touched][!cov][!aos];
  const dim3 grid((N + LR_PBWD_ROWS - 1) / LR_PBWD_ROWS), block(256);
  const float4* rows4 = reinterpret_cast<const float4*>(a.rows);
  lr_prof_begin(LRK_PROJECT_BWD, s);
  if (list) {
    lr_launch_zero_floats(a.o_mean2d, 3 * (size_t)N, s);
    float4* rows_w = const_cast<float4*>(rows4);   // (the accumulator rows are the caller's scratch: slots 12-15 are this path's)
    lr_launch_zero_words(reinterpret_cast<uint32_t*>(rows_w + 3), 4, s);
    hipLaunchKernelGGL(lr_pbwd_compact_kernel, dim3((N + LR_PBWD_CHUNK - 1) / LR_PBWD_CHUNK), dim3(1024), 0, s, a.pw, N, rows_w);
    hipLaunchKernelGGL(list_kernel[!a.sink_rows], dim3(2048), block, 0, s, v, N, a.means, a.scales, a.rots, rows_w, a.o_mean2d,
                       a.o_opac, a.o_col, a.g_means3d, a.g_scales, a.g_rots);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, v, N, a.means, a.scales, a.rots, a.radii, a.g_mean2d, a.g_conic, rows4,
                       a.o_mean2d, a.o_opac, a.o_col, a.pw, a.g_means3d, a.g_scales, a.g_rots, clear_inside, a.o_aux,
                       a.cam_partials, a.o_abs);
    if (cam) lr_launch_camera_finish(a.cam_partials, N, a.cam_dv, a.cam_dp, s);
  }
  lr_prof_end(LRK_PROJECT_BWD, s);
}
