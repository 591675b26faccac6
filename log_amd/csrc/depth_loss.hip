// depth_loss.hip -- the depth term of LoG's depth-supervised training (LoG/render/renderer.py:268-292 append_depth_loss,
// LoG/render/loss.py:47-117 ScaleAndShiftInvariantLoss at alpha = 0.5, one gradient scale): n patches of 64 x 64 pixels
// at device-resident positions, per patch the least-squares scale s and shift h of p = 1 / (pred + eps) onto gt over the
// pixels with acc > threshold, then
//   loss = (sum_k sum (m (s p + h - gt))^2 + alpha * sum_k sum over neighbour pairs m m' |d' - d|) / sum_k sum m.
// The reference slices the patches with device scalars (384 read-backs), stacks them and runs ~60 small kernels plus
// their autograd backward; here: one forward kernel (a workgroup per patch) + a one-workgroup sum, and one backward kernel.
//
// All arithmetic is double: the determinant a00 a11 - a01^2 of the 2 x 2 normal equations cancels to round-off in fp32 on
// patches of nearly constant depth, and 64 x 4096 pixels of double cost nothing that can be measured.  Inputs and outputs
// are fp32, read through their (y, x) element strides.
//
// Records (doubles, DL_REC per slot): slot 0 is the header {M, alpha, eps, threshold, n}, slot 1 + k belongs to patch k:
//   {r, c, a00, a01, a11, b0, b1, det, s, h, D, R, M*G0, M*G1, valid}  (G0 = sum g_j, G1 = sum g_j p_j, g_j = dloss/d(s p_j + h)).
// The backward needs nothing else: positions, sums, scale and shift all come from there.
//
// Bounds.  rows / cols are device data nobody reads on the host: a patch that does not lie inside the image is not
// loaded at all, its record says valid = 0, the loss becomes nan and the backward skips it.
//
// Determinism: per-thread sums in pixel order, a shuffle tree over the lanes, the four waves in order, the patches in
// patch order; the backward writes every element of grad_pred exactly once (patch order per pixel) -- no atomics, no memset.
#include "common.hpp"
#include "launch.hpp"

#define DL_THREADS 256
#define DL_ROWS (DL_PATCH * DL_PATCH / DL_THREADS)      // 16 pixels per thread: column tid % 64, rows 16 * wave ..
#define DL_TILE_H 16                                     // backward: a workgroup owns 64 x 16 image pixels
#define DL_TILE_ROWS (DL_TILE_H * DL_PATCH / DL_THREADS) // 4 pixels per thread

size_t lr_depth_loss_record_bytes(int n) { return n < 1 ? 0 : (size_t)(n + 1) * DL_REC * sizeof(double); }

// sums of NV values over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; every thread
// gets the result.  ws: NV * 4 doubles.
template <int NV>
LR_DEV void dl_block_sum(double (&v)[NV], double* ws) {
#pragma unroll
  for (int i = 0; i < NV; i++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[i] += __shfl_down(v[i], d);
  }
  __syncthreads();                                       // the previous use of ws is over
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int i = 0; i < NV; i++) ws[i * 4 + (threadIdx.x >> 6)] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; i++) v[i] = ((ws[i * 4] + ws[i * 4 + 1]) + ws[i * 4 + 2]) + ws[i * 4 + 3];
}

LR_DEV double dl_sign(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// The least-squares solution of one patch from its five sums; det == 0 (an empty patch, a patch with one valid pixel):
// s = h = 0, as compute_scale_and_shift leaves them.
LR_DEV void dl_solve(double a00, double a01, double a11, double b0, double b1, double& det, double& s, double& h) {
  det = a00 * a11 - a01 * a01;
  s = 0.0; h = 0.0;
  if (det != 0.0) {
    s = (a11 * b0 - a01 * b1) / det;
    h = (a00 * b1 - a01 * b0) / det;
  }
}

__global__ void __launch_bounds__(DL_THREADS)
depth_loss_fwd_kernel(DepthLossArgs a, const int64_t* __restrict__ rows, const int64_t* __restrict__ cols, double alpha,
                      double eps, double thr, double* __restrict__ records) {
  __shared__ double sd[DL_PATCH * DL_PATCH];             // d = m (s p + h - gt), for the neighbour differences
  __shared__ uint8_t sm[DL_PATCH * DL_PATCH];            // m
  __shared__ double ws[5 * 4];
  const int tid = (int)threadIdx.x, x = tid & 63, yb = (tid >> 6) * DL_ROWS;
  double* rec = records + (size_t)(1 + blockIdx.x) * DL_REC;
  const int64_t r = rows[blockIdx.x], c = cols[blockIdx.x];
  if (r < 0 || r > (int64_t)a.H - DL_PATCH || c < 0 || c > (int64_t)a.W - DL_PATCH) {     // uniform: nothing is loaded
    if (tid < DL_REC) rec[tid] = 0.0;
    return;
  }
  const float* pp = a.pred + (r * a.ps[0] + (c + x) * a.ps[1]);
  const float* gp = a.gt + (r * a.gs[0] + (c + x) * a.gs[1]);
  const float* ap = a.acc + (r * a.as[0] + (c + x) * a.as[1]);
  float fp[DL_ROWS], ft[DL_ROWS], fa[DL_ROWS];
#pragma unroll
  for (int i = 0; i < DL_ROWS; i++) {                    // all loads requested before the first is used
    fp[i] = pp[(int64_t)(yb + i) * a.ps[0]];
    ft[i] = gp[(int64_t)(yb + i) * a.gs[0]];
    fa[i] = ap[(int64_t)(yb + i) * a.as[0]];
  }
  double p[DL_ROWS];
  uint32_t mbits = 0;
  double v5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < DL_ROWS; i++) {
    p[i] = 1.0 / ((double)fp[i] + eps);
    if ((double)fa[i] > thr) {
      mbits |= 1u << i;
      const double t = (double)ft[i];
      v5[0] += p[i] * p[i]; v5[1] += p[i]; v5[2] += 1.0; v5[3] += p[i] * t; v5[4] += t;
    }
  }
  dl_block_sum<5>(v5, ws);
  double det, s, h;
  dl_solve(v5[0], v5[1], v5[2], v5[3], v5[4], det, s, h);

  double d[DL_ROWS];
#pragma unroll
  for (int i = 0; i < DL_ROWS; i++) {
    const bool m = (mbits >> i) & 1u;
    d[i] = m ? (s * p[i] + h) - (double)ft[i] : 0.0;
    sd[(yb + i) * DL_PATCH + x] = d[i];
    sm[(yb + i) * DL_PATCH + x] = m ? 1 : 0;
  }
  __syncthreads();
  double v4[4] = {0.0, 0.0, 0.0, 0.0};                   // D, R, M*G0, M*G1
#pragma unroll
  for (int i = 0; i < DL_ROWS; i++) {
    if (!((mbits >> i) & 1u)) continue;
    const int y = yb + i, o = y * DL_PATCH + x;
    double sg = 0.0;
    if (x + 1 < DL_PATCH && sm[o + 1]) { const double df = sd[o + 1] - d[i]; v4[1] += fabs(df); sg -= dl_sign(df); }
    if (y + 1 < DL_PATCH && sm[o + DL_PATCH]) { const double df = sd[o + DL_PATCH] - d[i]; v4[1] += fabs(df); sg -= dl_sign(df); }
    if (x > 0 && sm[o - 1]) sg += dl_sign(d[i] - sd[o - 1]);
    if (y > 0 && sm[o - DL_PATCH]) sg += dl_sign(d[i] - sd[o - DL_PATCH]);
    const double q = 2.0 * d[i] + alpha * sg;
    v4[0] += d[i] * d[i]; v4[2] += q; v4[3] += q * p[i];
  }
  dl_block_sum<4>(v4, ws);
  if (tid == 0) {
    rec[0] = (double)r; rec[1] = (double)c;
    rec[2] = v5[0]; rec[3] = v5[1]; rec[4] = v5[2]; rec[5] = v5[3]; rec[6] = v5[4];
    rec[7] = det; rec[8] = s; rec[9] = h;
    rec[10] = v4[0]; rec[11] = v4[1]; rec[12] = v4[2]; rec[13] = v4[3];
    rec[14] = 1.0; rec[15] = 0.0;
  }
}

// one workgroup: thread k fetches patch k's three numbers, thread 0 adds them in patch order
__global__ void __launch_bounds__(DL_MAX_PATCHES)
depth_loss_sum_kernel(int n, double alpha, double eps, double thr, double* __restrict__ records, void* __restrict__ out) {
  __shared__ double sD[DL_MAX_PATCHES], sR[DL_MAX_PATCHES], sM[DL_MAX_PATCHES], sV[DL_MAX_PATCHES];
  const int k = (int)threadIdx.x;
  if (k < n) {
    const double* rec = records + (size_t)(1 + k) * DL_REC;
    sD[k] = rec[10]; sR[k] = rec[11]; sM[k] = rec[4]; sV[k] = rec[14];
  }
  __syncthreads();
  if (k != 0) return;
  double D = 0.0, R = 0.0, M = 0.0;
  bool valid = true;
  for (int i = 0; i < n; i++) { D += sD[i]; R += sR[i]; M += sM[i]; valid = valid && sV[i] != 0.0; }
  const double loss = valid ? (D + alpha * R) / M : __builtin_nan("");      // M == 0: 0 / 0 = nan, as the reference
  *reinterpret_cast<float*>(out) = (float)loss;
  reinterpret_cast<double*>(out)[1] = M;
  records[0] = M; records[1] = alpha; records[2] = eps; records[3] = thr; records[4] = (double)n;
}

struct DlPixel { double p, t; bool m; };

LR_DEV DlPixel dl_load(const DepthLossArgs& a, int y, int x, double eps, double thr) {
  DlPixel q = {0.0, 0.0, false};
  if (y < 0 || y >= a.H || x < 0 || x >= a.W) return q;
  q.m = (double)a.acc[(int64_t)y * a.as[0] + (int64_t)x * a.as[1]] > thr;
  if (q.m) {
    q.p = 1.0 / ((double)a.pred[(int64_t)y * a.ps[0] + (int64_t)x * a.ps[1]] + eps);
    q.t = (double)a.gt[(int64_t)y * a.gs[0] + (int64_t)x * a.gs[1]];
  }
  return q;
}

__global__ void __launch_bounds__(DL_THREADS)
depth_loss_bwd_kernel(DepthLossArgs a, int n, const double* __restrict__ records, const float* __restrict__ grad_loss,
                      float* __restrict__ grad_pred) {
  __shared__ double srec[DL_MAX_PATCHES * DL_REC];       // the records of the patches that reach this tile, in patch order
  __shared__ int shit[DL_MAX_PATCHES];
  __shared__ int scount[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = (int)blockIdx.x * DL_PATCH, y0 = (int)blockIdx.y * DL_TILE_H;

  // which patches reach the tile (valid, det != 0): ordered compaction -- ballot inside a wave, the waves in order
  bool hit = false;
  if (tid < n) {
    const double* rec = records + (size_t)(1 + tid) * DL_REC;
    const double r = rec[0], c = rec[1];
    hit = rec[14] != 0.0 && rec[7] != 0.0 && r < (double)(y0 + DL_TILE_H) && r + DL_PATCH > (double)y0 &&
          c < (double)(x0 + DL_PATCH) && c + DL_PATCH > (double)x0;
  }
  const uint64_t ballot = __ballot(hit);
  if (lane == 0) scount[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, nhit = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) { if (w < wave) before += scount[w]; nhit += scount[w]; }
  if (hit) shit[before + __popcll(ballot & ((1ull << lane) - 1ull))] = tid;
  __syncthreads();
  for (int i = tid; i < nhit * DL_REC; i += DL_THREADS) srec[i] = records[(size_t)(1 + shit[i / DL_REC]) * DL_REC + (i % DL_REC)];
  __syncthreads();

  const double M = records[0], alpha = records[1], eps = records[2], thr = records[3];
  const double gl = (double)grad_loss[0];
  const int x = x0 + lane;
  if (x >= a.W) return;
#pragma unroll 1
  for (int j = 0; j < DL_TILE_ROWS; j++) {
    const int y = y0 + wave + 4 * j;
    if (y >= a.H) break;
    float out = 0.f;                                     // pixels no patch covers and pixels with m = 0: an exact 0
    if (nhit > 0) {
      const DlPixel ce = dl_load(a, y, x, eps, thr);
      if (ce.m) {
        const DlPixel le = dl_load(a, y, x - 1, eps, thr), ri = dl_load(a, y, x + 1, eps, thr);
        const DlPixel up = dl_load(a, y - 1, x, eps, thr), dn = dl_load(a, y + 1, x, eps, thr);
        double acc = 0.0;
        bool any = false;
        for (int i = 0; i < nhit; i++) {
          const double* rec = srec + i * DL_REC;
          const int r = (int)rec[0], c = (int)rec[1];
          if (y < r || y >= r + DL_PATCH || x < c || x >= c + DL_PATCH) continue;
          any = true;
          const double a01 = rec[3], a11 = rec[4], b0 = rec[5], b1 = rec[6], det = rec[7], s = rec[8], h = rec[9];
          const double d = (s * ce.p + h) - ce.t;
          double sg = 0.0;
          if (x + 1 < c + DL_PATCH && ri.m) sg -= dl_sign(((s * ri.p + h) - ri.t) - d);
          if (y + 1 < r + DL_PATCH && dn.m) sg -= dl_sign(((s * dn.p + h) - dn.t) - d);
          if (x > c && le.m) sg += dl_sign(d - ((s * le.p + h) - le.t));
          if (y > r && up.m) sg += dl_sign(d - ((s * up.p + h) - up.t));
          const double q = 2.0 * d + alpha * sg;                          // M * g_j
          const double ddet = 2.0 * a11 * ce.p - 2.0 * a01;
          const double ds = ((a11 * ce.t - b1) - s * ddet) / det;
          const double dh = ((2.0 * ce.p * b1 - b0 - a01 * ce.t) - h * ddet) / det;
          acc += s * q + rec[13] * ds + rec[12] * dh;                     // M * dloss/dp_j of this patch
        }
        if (any) out = (float)((-(ce.p * ce.p) * (acc / M)) * gl);
      }
    }
    grad_pred[(int64_t)y * a.W + x] = out;
  }
}

hipError_t lr_launch_depth_loss_fwd(const DepthLossArgs& a, int n, const int64_t* rows, const int64_t* cols, double alpha,
                                    double eps, double thr, void* out, double* records, hipStream_t s) {
  hipLaunchKernelGGL(depth_loss_fwd_kernel, dim3((uint32_t)n), dim3(DL_THREADS), 0, s, a, rows, cols, alpha, eps, thr, records);
  hipLaunchKernelGGL(depth_loss_sum_kernel, dim3(1), dim3(DL_MAX_PATCHES), 0, s, n, alpha, eps, thr, records, out);
  return hipGetLastError();
}

hipError_t lr_launch_depth_loss_bwd(const DepthLossArgs& a, int n, const double* records, const float* grad_loss,
                                    float* grad_pred, hipStream_t s) {
  const dim3 grid((uint32_t)((a.W + DL_PATCH - 1) / DL_PATCH), (uint32_t)((a.H + DL_TILE_H - 1) / DL_TILE_H));
  hipLaunchKernelGGL(depth_loss_bwd_kernel, grid, dim3(DL_THREADS), 0, s, a, n, records, grad_loss, grad_pred);
  return hipGetLastError();
}
