// pose.hip -- a per-view pose correction applied to a camera (log_amd/pose.py: PoseTable.camera) and its backward.
// A row of the table is xi = (omega[3], upsilon[3]): the camera-frame perturbation p_cam' = R(omega) p_cam + upsilon with
// R(omega) = I + A K + B K^2 (Rodrigues; K = [omega]x, s = |omega|^2, A = sin(sqrt s) / sqrt s, B = (1 - cos(sqrt s)) / s, both by
// their series below LR_POSE_SERIES).  In the row-vector convention of the rasterizer (p_cam = [p 1] V):
//   E  = [[R^T - I, 0], [upsilon, 0]]            (D = I + E is the perturbation as a 4x4)
//   W  = V E,  V' = V + W,  P' = P + W M,  M = V^-1 P
//   V^-1 = [[A3^T, 0], [-b A3^T, 1]] for V = [[A3, 0], [b, 1]] (the rigid closed form),  campos' = -b' A3'^T (row 3 of V'^-1)
// -- V D and V' (V^-1 P) written as differences from the inputs, so that xi = 0 returns V and P to the bit whatever the
// rounding of V^-1.  Everything is evaluated in double from the fp32 inputs and rounded once.  Both kernels are one wave:
// the work is ~300 double operations, uniform over the lanes (every lane computes all of it; lanes 0..15 / 0..5 store).
#include "common.hpp"
#include "launch.hpp"

#define LR_POSE_SERIES 1e-2   // s below this: the series (first dropped terms below 1e-16 there; above it the closed forms'
                              // cancellation, 1e-16 / s, costs less than 1e-11 of a derivative)

struct LrPose {
  double R[9];        // R(omega), row-major
  double A, B, dA, dB;   // the two coefficients and their derivatives in s
  double w[3], u[3];
};

LR_DEV void lr_pose_load(const float* __restrict__ row, LrPose& q) {
#pragma unroll
  for (int k = 0; k < 3; k++) { q.w[k] = (double)row[k]; q.u[k] = (double)row[3 + k]; }
  const double s = q.w[0] * q.w[0] + q.w[1] * q.w[1] + q.w[2] * q.w[2];
  if (s < LR_POSE_SERIES) {
    q.A = 1.0 + s * (-1.0 / 6.0 + s * (1.0 / 120.0 + s * (-1.0 / 5040.0 + s * (1.0 / 362880.0))));
    q.B = 0.5 + s * (-1.0 / 24.0 + s * (1.0 / 720.0 + s * (-1.0 / 40320.0 + s * (1.0 / 3628800.0))));
    q.dA = -1.0 / 6.0 + s * (1.0 / 60.0 + s * (-1.0 / 1680.0 + s * (1.0 / 90720.0)));
    q.dB = -1.0 / 24.0 + s * (1.0 / 360.0 + s * (-1.0 / 13440.0 + s * (1.0 / 907200.0)));
  } else {
    const double th = sqrt(s), sn = sin(th), cs = cos(th), hs = sin(0.5 * th) / (0.5 * th);
    q.A = sn / th;
    q.B = 0.5 * hs * hs;   // (1 - cos th) / s without the cancellation
    q.dA = (cs - q.A) / (2.0 * s);
    q.dB = (0.5 * q.A - q.B) / s;
  }
  const double x = q.w[0], y = q.w[1], z = q.w[2];
  // K = [[0, -z, y], [z, 0, -x], [-y, x, 0]];  K^2 = omega omega^T - s I
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++)
      q.R[3 * a + b] = (a == b ? 1.0 : 0.0) + q.A * K[3 * a + b] + q.B * (q.w[a] * q.w[b] - (a == b ? s : 0.0));
}

// E = D - I, row-major 4x4 (column 3 is zero): E[b][a] = R[a][b] - delta, E[3][k] = upsilon[k]
LR_DEV void lr_pose_E(const LrPose& q, double E[16]) {
  const double x = q.w[0], y = q.w[1], z = q.w[2];
  const double s = x * x + y * y + z * z;
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
#pragma unroll
  for (int i = 0; i < 16; i++) E[i] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++)   // (R - I without the cancellation of computing R first)
      E[4 * b + a] = q.A * K[3 * a + b] + q.B * (q.w[a] * q.w[b] - (a == b ? s : 0.0));
#pragma unroll
  for (int k = 0; k < 3; k++) E[12 + k] = q.u[k];
}

// M = V^-1 P with the rigid closed form of V^-1
LR_DEV void lr_pose_M(const double V[16], const double P[16], double M[16]) {
  double Vi[16];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) Vi[4 * i + k] = V[4 * k + i];
    Vi[4 * i + 3] = 0.0;
    Vi[12 + i] = -(V[12] * V[4 * i] + V[13] * V[4 * i + 1] + V[14] * V[4 * i + 2]);
  }
  Vi[15] = 1.0;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      M[4 * r + c] = Vi[4 * r] * P[c] + Vi[4 * r + 1] * P[4 + c] + Vi[4 * r + 2] * P[8 + c] + Vi[4 * r + 3] * P[12 + c];
}

LR_DEV void lr_mat4(const double A[16], const double B[16], double C[16]) {
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * B[12 + c];
}

__global__ void __launch_bounds__(64)
lr_pose_apply_kernel(const float* __restrict__ table, int index, const float* __restrict__ view,
                     const float* __restrict__ proj, float* __restrict__ view_out, float* __restrict__ proj_out,
                     float* __restrict__ campos_out) {
  const int tid = (int)threadIdx.x;
  LrPose q;
  lr_pose_load(table + 6 * (size_t)index, q);
  double V[16], P[16], E[16], M[16], W[16], WM[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { V[i] = (double)view[i]; P[i] = (double)proj[i]; }
  lr_pose_E(q, E);
  lr_pose_M(V, P, M);
  lr_mat4(V, E, W);
  lr_mat4(W, M, WM);
  double Vn[16];
#pragma unroll
  for (int i = 0; i < 16; i++) Vn[i] = V[i] + W[i];
  double cp[3];
#pragma unroll
  for (int i = 0; i < 3; i++) cp[i] = -(Vn[12] * Vn[4 * i] + Vn[13] * Vn[4 * i + 1] + Vn[14] * Vn[4 * i + 2]);
  // (stores through a select over unrolled indices: the arrays stay in registers)
#pragma unroll
  for (int i = 0; i < 16; i++)
    if (tid == i) { view_out[i] = (float)Vn[i]; proj_out[i] = (float)(P[i] + WM[i]); }
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (tid == i) campos_out[i] = (float)cp[i];
}

// dL/dxi of row `index`, ADDED into grad[index]: g_view / g_proj [4, 4] and g_campos [3] are dL/dV', dL/dP', dL/dcampos'
// (any of them may be NULL = zeros).  V and P are constants of the function.
__global__ void __launch_bounds__(64)
lr_pose_backward_kernel(const float* __restrict__ table, int index, const float* __restrict__ view,
                        const float* __restrict__ proj, const float* __restrict__ g_view, const float* __restrict__ g_proj,
                        const float* __restrict__ g_campos, float* __restrict__ grad) {
  const int tid = (int)threadIdx.x;
  LrPose q;
  lr_pose_load(table + 6 * (size_t)index, q);
  double V[16], P[16], M[16], G[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { V[i] = (double)view[i]; P[i] = (double)proj[i]; }
  lr_pose_M(V, P, M);
  // G = dL/dW = dL/dV' + dL/dP' M^T (+ the campos' path below)
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      double g = g_view ? (double)g_view[4 * r + c] : 0.0;
      if (g_proj)
        g += (double)g_proj[4 * r] * M[4 * c] + (double)g_proj[4 * r + 1] * M[4 * c + 1] + (double)g_proj[4 * r + 2] * M[4 * c + 2] +
             (double)g_proj[4 * r + 3] * M[4 * c + 3];
      G[4 * r + c] = g;
    }
  if (g_campos) {   // campos'_i = -sum_k b'_k A'[i][k]: needs V' itself
    double E[16], W[16];
    lr_pose_E(q, E);
    lr_mat4(V, E, W);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double gc = (double)g_campos[i];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        G[4 * i + k] -= gc * (V[12 + k] + W[12 + k]);
        G[12 + k] -= gc * (V[4 * i + k] + W[4 * i + k]);
      }
    }
  }
  // dL/dE = V^T G;  dL/dupsilon_k = (V^T G)[3][k];  dL/dR[a][b] = (V^T G)[b][a]
  double gE[16];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      gE[4 * r + c] = V[r] * G[c] + V[4 + r] * G[4 + c] + V[8 + r] * G[8 + c] + V[12 + r] * G[12 + c];
  double gR[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) gR[3 * a + b] = gE[4 * b + a];
  // R = I + A K + B (w w^T - s I): with gK = sum gR .* dK, S = sum_ab gR[a][b] K[a][b], Q = w^T gR w - s tr gR
  //   dL/dw_i = 2 w_i (dA S + dB Q) + A gK_i + B (((gR + gR^T) w)_i - 2 w_i tr gR)
  const double x = q.w[0], y = q.w[1], z = q.w[2];
  const double s = x * x + y * y + z * z;
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
  double S = 0.0, tr = gR[0] + gR[4] + gR[8], wgw = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) { S += gR[3 * a + b] * K[3 * a + b]; wgw += q.w[a] * gR[3 * a + b] * q.w[b]; }
  const double Q = wgw - s * tr;
  const double gK[3] = {gR[7] - gR[5], gR[2] - gR[6], gR[3] - gR[1]};   // d/dx, d/dy, d/dz of sum gR .* K
  double out[6];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double sym = (gR[3 * i] + gR[i]) * x + (gR[3 * i + 1] + gR[3 + i]) * y + (gR[3 * i + 2] + gR[6 + i]) * z;
    out[i] = 2.0 * q.w[i] * (q.dA * S + q.dB * Q) + q.A * gK[i] + q.B * (sym - 2.0 * q.w[i] * tr);
    out[3 + i] = gE[12 + i];
  }
  float* const g = grad + 6 * (size_t)index;
#pragma unroll
  for (int i = 0; i < 6; i++)
    if (tid == i) g[i] += (float)out[i];
}

hipError_t lr_launch_pose_apply(const float* table, int index, const float* view, const float* proj, float* view_out,
                                float* proj_out, float* campos_out, hipStream_t s) {
  hipLaunchKernelGGL(lr_pose_apply_kernel, dim3(1), dim3(64), 0, s, table, index, view, proj, view_out, proj_out, campos_out);
  return hipGetLastError();
}

hipError_t lr_launch_pose_backward(const float* table, int index, const float* view, const float* proj, const float* g_view,
                                   const float* g_proj, const float* g_campos, float* grad, hipStream_t s) {
  hipLaunchKernelGGL(lr_pose_backward_kernel, dim3(1), dim3(64), 0, s, table, index, view, proj, g_view, g_proj, g_campos, grad);
  return hipGetLastError();
}
