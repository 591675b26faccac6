// evaluate.hip -- what a validation image costs after it is rendered (LoG/utils/trainer.py:313-332 make_validation,
// LoG/utils/metric.py psnr / ssim, LoG/render/renderer.py:19-23 tensor_to_bgr): the view-correction fit over the left
// half, gain and clamp, L1, the squared error behind the PSNR, the metric's SSIM and the 8-bit BGR export -- in
//   eval_gain_kernel + eval_gain_reduce_kernel   (only with the fit),
//   eval_metrics_kernel<SSIM, GAIN> + eval_metrics_reduce_kernel,
//   eval_bgr8_kernel<C>                          (the export on its own: demo, validate_for_metric),
// and ONE read-back of a 128-byte record instead of seven full-image reductions, an .item() and a float32 copy of the
// image to the host.
//
// Images are fp32 [C, H, W] read through three element strides (c, y, x), so a view of an HWC batch image is read in place;
// inside a plane y * sy + x * sx fits 32 bits (checked by the entry points).
//
// eval_metrics_kernel.  A workgroup of 256 threads owns a 32 x 32 tile of one channel plane, as loss_fwd_kernel does.  Per
// pixel p = GAIN ? clamp(fp32(gain[c] * pred), 0, 1) : pred (a nan stays a nan) and d = p - gt; the owner of a pixel adds
// |d| and d * d (fp32 operations, as the reference's) into double sums, writes p to `corrected` and the bytes of p and gt to
// `bgr8`, each where asked.  With SSIM the tile is staged with a halo of 5 on every side -- ZERO outside the image: metric.py pads, so
// there are H x W outputs -- and the 11-tap window (sigma 1.5) runs horizontally for the five moments, then vertically with
// four output rows per thread; the moments are taken of (x - 0.5) as in loss.hip (the same real numbers, less cancellation;
// a padded tap holds -0.5).  Then metric.py:91-101: variances clamped at 0, the covariance limited to sqrt(s00 * s11).
// LDS: 42 x 42 float2 + 2 x (42 x 32 float2) + the sums' scratch = 35 712 bytes (e01 of the horizontal pass goes over the
// consumed input tile; loss_fwd_kernel: 35 648): four workgroups per CU of 160 KiB.  Without SSIM the kernel uses no LDS beyond the sums' scratch.
//
// Determinism: every workgroup leaves its sums as doubles in its own slot; one workgroup adds the slots in a fixed order in
// double.  No floating-point atomics; every store is a plain vector store.  The same input gives the same bits.
//
// Record (16 doubles): [0] sum |d|  [1] sum d^2  [2] sum ssim_map  [3] element count C * H * W  [4..7] gain[c] (the fp32
// value; 1 without the fit, 0 for c >= C)  [8..11] sum gt * pred over the left half  [12..15] sum pred^2 over the left half.
#include "common.hpp"
#include "launch.hpp"

#define EV_T 32
#define EV_PAD 5
#define EV_IN (EV_T + 2 * EV_PAD)
#define EV_THREADS 256
#define EV_ROWS 4
#define EV_CENTER 0.5f
#define EV_STAGE ((EV_IN * EV_IN + EV_THREADS - 1) / EV_THREADS)    // 7
#define EV_HITEMS ((EV_IN * EV_T + EV_THREADS - 1) / EV_THREADS)    // 6
#define EV_GAIN_PER_THREAD 16
#define EV_GAIN_BLOCK (EV_THREADS * EV_GAIN_PER_THREAD)             // left-half elements per workgroup of the fit
#define EV_RED_THREADS 256

static inline size_t ev_metric_blocks(int C, int H, int W) {
  return (size_t)((W + EV_T - 1) / EV_T) * (size_t)((H + EV_T - 1) / EV_T) * (size_t)C;
}
static inline size_t ev_gain_blocks(int H, int W) {
  return ((size_t)H * (size_t)(W / 2) + EV_GAIN_BLOCK - 1) / EV_GAIN_BLOCK;
}

// [2 * C * gain blocks] doubles of the fit, then [3 * metric blocks] doubles of the metrics
size_t lr_eval_scratch_bytes(int C, int H, int W) {
  if (C < 1 || C > 4 || H < 1 || W < 1) return 0;
  const size_t bytes = 8 * (2 * (size_t)C * ev_gain_blocks(H, W) + 3 * ev_metric_blocks(C, H, W));
  return (bytes + 255) & ~(size_t)255;
}

// the 8-bit form of renderer.py:21: clip to [0, 1], times 255 in fp32, truncate
LR_DEV uint32_t ev_byte(float v) { return (uint32_t)(int)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// torch.clamp(v, 0, 1): a nan stays a nan (a fit over an empty or all-zero left half gives one, as in the reference)
LR_DEV float ev_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// sum over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; valid in thread 0
LR_DEV double ev_block_sum(double v, double* ws) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// thread t adds slots t, t + 256, ... of p[i * stride], then a fixed tree over the threads; valid in thread 0
LR_DEV double ev_slot_sum(const double* __restrict__ p, uint32_t n, uint32_t stride, double* s) {
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += EV_RED_THREADS) acc += p[(size_t)i * stride];
  __syncthreads();                                          // the previous sum's s[0] has been read
  s[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t d = EV_RED_THREADS / 2; d >= 1; d >>= 1) {
    if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  return s[0];
}

// ---- the view-correction fit: sum gt * pred and sum pred^2 over columns [0, W / 2) per channel --------------------
__global__ void __launch_bounds__(EV_THREADS)
eval_gain_kernel(EvalArgs a, uint32_t nblk) {
  __shared__ double ws[8];
  const int c = (int)(blockIdx.x / nblk);
  const uint32_t blk = blockIdx.x - (uint32_t)c * nblk;
  const int Wh = a.W / 2;
  const uint32_t n = (uint32_t)a.H * (uint32_t)Wh;
  const float* pp = a.pred + (int64_t)c * a.ps[0];
  const float* gp = a.gt + (int64_t)c * a.gs[0];
  const int psy = (int)a.ps[1], psx = (int)a.ps[2], gsy = (int)a.gs[1], gsx = (int)a.gs[2];
  float pv[EV_GAIN_PER_THREAD], gv[EV_GAIN_PER_THREAD];
#pragma unroll
  for (int u = 0; u < EV_GAIN_PER_THREAD; u++) {
    const uint32_t i = blk * EV_GAIN_BLOCK + (uint32_t)u * EV_THREADS + threadIdx.x;
    const bool in = i < n;
    const int y = in ? (int)(i / (uint32_t)Wh) : 0, x = in ? (int)(i - (uint32_t)y * (uint32_t)Wh) : 0;
    pv[u] = in ? pp[y * psy + x * psx] : 0.f;
    gv[u] = in ? gp[y * gsy + x * gsx] : 0.f;
  }
  double sgp = 0.0, spp = 0.0;
#pragma unroll
  for (int u = 0; u < EV_GAIN_PER_THREAD; u++) {
    sgp += (double)gv[u] * (double)pv[u];
    spp += (double)pv[u] * (double)pv[u];
  }
  const double b0 = ev_block_sum(sgp, ws);
  const double b1 = ev_block_sum(spp, ws + 4);
  if (threadIdx.x == 0) {
    double* out = a.gain_partial + 2 * (size_t)blockIdx.x;
    out[0] = b0; out[1] = b1;
  }
}

__global__ void __launch_bounds__(EV_RED_THREADS)
eval_gain_reduce_kernel(const double* __restrict__ partial, int C, uint32_t nblk, double* __restrict__ record) {
  __shared__ double s[EV_RED_THREADS];
  for (int c = 0; c < 4; c++) {
    double sgp = 0.0, spp = 0.0;
    if (c < C) {
      sgp = ev_slot_sum(partial + 2 * (size_t)c * nblk, nblk, 2, s);
      spp = ev_slot_sum(partial + 2 * (size_t)c * nblk + 1, nblk, 2, s);
    }
    if (threadIdx.x == 0) {
      record[4 + c] = c < C ? (double)(float)(sgp / spp) : 0.0;     // 0 / 0 = nan, x / 0 = inf: as the reference's division
      record[8 + c] = sgp;
      record[12 + c] = spp;
    }
  }
}

// ---- the metrics ---------------------------------------------------------------------------------------------------
template <bool SSIM, bool GAIN>
__global__ void __launch_bounds__(EV_THREADS)
eval_metrics_kernel(EvalArgs a) {
  __shared__ double ws[12];
  const int tid = (int)threadIdx.x;
  int t = (int)blockIdx.x;
  const int c = t % a.C; t /= a.C;
  const int tx = t % a.ntx;
  const int ty = t / a.ntx;
  const int x0 = tx * EV_T, y0 = ty * EV_T;
  const float* pp = a.pred + (int64_t)c * a.ps[0];
  const float* gp = a.gt + (int64_t)c * a.gs[0];
  const int psy = (int)a.ps[1], psx = (int)a.ps[2], gsy = (int)a.gs[1], gsx = (int)a.gs[2];
  float gain = 1.f;
  if constexpr (GAIN) gain = (float)a.record[4 + c];
  float* corr = a.corrected ? a.corrected + (int64_t)c * ((int64_t)a.H * a.W) : nullptr;
  uint8_t* b8p = a.bgr8 ? a.bgr8 + (a.C - 1 - c) : nullptr;                 // the corrected image's rows, channels reversed
  uint8_t* b8g = a.bgr8 ? b8p + (int64_t)a.H * a.W * a.C : nullptr;         // ... and the ground truth's below them

  double sl1 = 0.0, sd2 = 0.0, sss = 0.0;
  // what the owner of pixel (y, x) does with it
  auto pixel = [&](int y, int x, float p, float g) {
    const float d = p - g;
    sl1 += (double)fabsf(d);
    sd2 += (double)(d * d);
    const int o = y * a.W + x;
    if (corr) corr[o] = p;
    if (b8p) {
      b8p[(int64_t)o * a.C] = (uint8_t)ev_byte(p);
      b8g[(int64_t)o * a.C] = (uint8_t)ev_byte(g);
    }
  };

  if constexpr (!SSIM) {
    const int x = x0 + (tid & (EV_T - 1)), yq = y0 + (tid / EV_T) * EV_ROWS;
    float pv[EV_ROWS], gv[EV_ROWS];
#pragma unroll
    for (int j = 0; j < EV_ROWS; j++) {
      const int y = yq + j;
      const bool in = x < a.W && y < a.H;
      pv[j] = in ? pp[y * psy + x * psx] : 0.f;
      gv[j] = in ? gp[y * gsy + x * gsx] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < EV_ROWS; j++) {
      const int y = yq + j;
      if (x >= a.W || y >= a.H) continue;
      float p = pv[j];
      if constexpr (GAIN) p = ev_clamp01(gain * p);
      pixel(y, x, p, gv[j]);
    }
  } else {
    __shared__ lr_f2 spg[EV_IN * EV_IN];                      // (p - 0.5, gt - 0.5); -0.5 where the reference pads with 0
    __shared__ lr_f2 hmu[EV_IN * EV_T], hee[EV_IN * EV_T];    // horizontal pass: (mu0, mu1), (e00, e11)
    float* he01 = reinterpret_cast<float*>(spg);              // ... and e01, over the input tile once it has been consumed

    float pv[EV_STAGE], gv[EV_STAGE];
#pragma unroll
    for (int u = 0; u < EV_STAGE; u++) {
      const int i = tid + u * EV_THREADS;
      const int ly = i / EV_IN, lx = i - ly * EV_IN;
      const int y = y0 - EV_PAD + ly, x = x0 - EV_PAD + lx;
      const bool in = i < EV_IN * EV_IN && y >= 0 && y < a.H && x >= 0 && x < a.W;
      pv[u] = in ? pp[y * psy + x * psx] : 0.f;
      gv[u] = in ? gp[y * gsy + x * gsx] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < EV_STAGE; u++) {
      const int i = tid + u * EV_THREADS;
      const int ly = i / EV_IN, lx = i - ly * EV_IN;
      const int y = y0 - EV_PAD + ly, x = x0 - EV_PAD + lx;
      const bool in = i < EV_IN * EV_IN && y >= 0 && y < a.H && x >= 0 && x < a.W;
      float p = pv[u];
      if constexpr (GAIN) { if (in) p = ev_clamp01(gain * p); }
      const bool own = in && lx >= EV_PAD && lx < EV_PAD + EV_T && ly >= EV_PAD && ly < EV_PAD + EV_T;
      if (own) pixel(y, x, p, gv[u]);
      if (i < EV_IN * EV_IN) spg[i] = lr_f2{p - EV_CENTER, gv[u] - EV_CENTER};
    }
    __syncthreads();

    // horizontal pass: 42 rows x 32 columns, five moments
    float e01v[EV_HITEMS];
#pragma unroll
    for (int u = 0; u < EV_HITEMS; u++) {
      const int i = tid + u * EV_THREADS;
      e01v[u] = 0.f;
      if (i < EV_IN * EV_T) {
        const int row = i / EV_T, hx = i - row * EV_T;
        const lr_f2* q = spg + row * EV_IN + hx;
        lr_f2 mu = {0.f, 0.f}, ee = {0.f, 0.f};
        float e01 = 0.f;
#pragma unroll
        for (int k = 0; k < LS_WIN_TAPS; k++) {
          const float w = a.w[k];
          const lr_f2 v = q[k], w2 = {w, w};
          mu = lr_fma2(w2, v, mu);
          ee = lr_fma2(w2, v * v, ee);
          e01 = lr_fma(w, v.x * v.y, e01);
        }
        hmu[i] = mu; hee[i] = ee; e01v[u] = e01;
      }
    }
    __syncthreads();                                          // every read of the input tile is done: e01 goes over it
#pragma unroll
    for (int u = 0; u < EV_HITEMS; u++) {
      const int i = tid + u * EV_THREADS;
      if (i < EV_IN * EV_T) he01[i] = e01v[u];
    }
    __syncthreads();

    // vertical pass: column xo, output rows yq .. yq+3 out of LDS rows yq .. yq+13
    const int xo = tid & (EV_T - 1), yq = (tid / EV_T) * EV_ROWS;
    lr_f2 amu[EV_ROWS], aee[EV_ROWS];
    float a01[EV_ROWS];
#pragma unroll
    for (int j = 0; j < EV_ROWS; j++) { amu[j] = lr_f2{0.f, 0.f}; aee[j] = lr_f2{0.f, 0.f}; a01[j] = 0.f; }
#pragma unroll
    for (int rr = 0; rr < EV_ROWS + 2 * EV_PAD; rr++) {
      const int o = (yq + rr) * EV_T + xo;
      const lr_f2 vmu = hmu[o], vee = hee[o];
      const float v01 = he01[o];
#pragma unroll
      for (int j = 0; j < EV_ROWS; j++) {
        const int k = rr - j;
        if (k >= 0 && k < LS_WIN_TAPS) {
          const lr_f2 w2 = {a.w[k], a.w[k]};
          amu[j] = lr_fma2(w2, vmu, amu[j]);
          aee[j] = lr_fma2(w2, vee, aee[j]);
          a01[j] = lr_fma(a.w[k], v01, a01[j]);
        }
      }
    }
    float ssum = 0.f;
#pragma unroll
    for (int j = 0; j < EV_ROWS; j++) {
      if (x0 + xo >= a.W || y0 + yq + j >= a.H) continue;
      const float m0c = amu[j].x, m1c = amu[j].y;
      const float s00 = fmaxf(aee[j].x - m0c * m0c, 0.f), s11 = fmaxf(aee[j].y - m1c * m1c, 0.f);
      const float r01 = a01[j] - m0c * m1c;
      const float lim = fminf(sqrtf(s00 * s11), fabsf(r01));
      const float s01 = r01 > 0.f ? lim : (r01 < 0.f ? -lim : 0.f);
      const float mu0 = m0c + EV_CENTER, mu1 = m1c + EV_CENTER;
      const float numer = lr_fma(2.f * mu0, mu1, a.c1) * lr_fma(2.f, s01, a.c2);
      const float denom = lr_fma(mu0, mu0, lr_fma(mu1, mu1, a.c1)) * ((s00 + s11) + a.c2);
      ssum += numer / denom;
    }
    sss = (double)ssum;
  }
  const double b0 = ev_block_sum(sl1, ws);
  const double b1 = ev_block_sum(sd2, ws + 4);
  const double b2 = SSIM ? ev_block_sum(sss, ws + 8) : 0.0;
  if (tid == 0) {
    double* out = a.partial + 3 * (size_t)blockIdx.x;
    out[0] = b0; out[1] = b1; out[2] = b2;
  }
}

__global__ void __launch_bounds__(EV_RED_THREADS)
eval_metrics_reduce_kernel(const double* __restrict__ partial, uint32_t blocks, int C, double count, int fit, double* __restrict__ record) {
  __shared__ double s[EV_RED_THREADS];
  for (int k = 0; k < 3; k++) {
    const double v = ev_slot_sum(partial + k, blocks, 3, s);
    if (threadIdx.x == 0) record[k] = v;
  }
  if (threadIdx.x == 0) {
    record[3] = count;
    if (!fit)
      for (int c = 0; c < 4; c++) { record[4 + c] = c < C ? 1.0 : 0.0; record[8 + c] = 0.0; record[12 + c] = 0.0; }
  }
}

// ---- the export on its own: [C, H, W] fp32 -> uint8 [H, W, C], channels reversed -------------------------------------
// A thread converts the four pixels 4 g .. 4 g + 3 of the flattened image and writes their 4 C bytes as C dwords (out is
// 4-byte aligned: checked by the entry point).  vec: x stride 1, W a multiple of 4 and every row start 16-byte aligned, so
// the four pixels are one 16-byte load per plane.
template <int C>
__global__ void __launch_bounds__(EV_THREADS)
eval_bgr8_kernel(EvalArgs a, uint32_t groups, int vec) {
  const uint32_t g = blockIdx.x * EV_THREADS + threadIdx.x;
  if (g >= groups) return;
  const uint32_t n = (uint32_t)a.H * (uint32_t)a.W, i0 = 4u * g;
  const int sy = (int)a.ps[1], sx = (int)a.ps[2];
  float v[C][4];
  if (vec) {
    const int y = (int)(i0 / (uint32_t)a.W), x = (int)(i0 - (uint32_t)y * (uint32_t)a.W);
#pragma unroll
    for (int c = 0; c < C; c++) {
      const float4 q = *reinterpret_cast<const float4*>(a.pred + (int64_t)c * a.ps[0] + (y * sy + x));
      v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = i0 + k;
      const bool in = i < n;
      const int y = in ? (int)(i / (uint32_t)a.W) : 0, x = in ? (int)(i - (uint32_t)y * (uint32_t)a.W) : 0;
#pragma unroll
      for (int c = 0; c < C; c++) v[c][k] = in ? a.pred[(int64_t)c * a.ps[0] + (y * sy + x * sx)] : 0.f;
    }
  }
  uint32_t word[C];
#pragma unroll
  for (int j = 0; j < C; j++) word[j] = 0u;
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int c = 0; c < C; c++) {
      const int byte = k * C + (C - 1 - c);
      word[byte >> 2] |= ev_byte(v[c][k]) << (8 * (byte & 3));
    }
  uint8_t* out = a.bgr8 + (size_t)i0 * C;
  if (i0 + 4u <= n) {
#pragma unroll
    for (int j = 0; j < C; j++) reinterpret_cast<uint32_t*>(out)[j] = word[j];
  } else {
    const uint32_t bytes = (n - i0) * C;                      // the image's last one to three pixels
#pragma unroll
    for (int j = 0; j < 4 * C; j++)
      if ((uint32_t)j < bytes) out[j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
  }
}

hipError_t lr_launch_eval_bgr8(const EvalArgs& a, hipStream_t s) {
  const uint32_t n = (uint32_t)a.H * (uint32_t)a.W, groups = (n + 3u) / 4u;
  const uint32_t blocks = (groups + EV_THREADS - 1) / EV_THREADS;
  bool vec = a.ps[2] == 1 && a.W % 4 == 0 && a.ps[1] % 4 == 0 && (reinterpret_cast<uintptr_t>(a.pred) & 15u) == 0;
  for (int c = 1; c < a.C; c++) vec = vec && a.ps[0] % 4 == 0;
  switch (a.C) {
    case 1: hipLaunchKernelGGL(eval_bgr8_kernel<1>, dim3(blocks), dim3(EV_THREADS), 0, s, a, groups, (int)vec); break;
    case 2: hipLaunchKernelGGL(eval_bgr8_kernel<2>, dim3(blocks), dim3(EV_THREADS), 0, s, a, groups, (int)vec); break;
    case 3: hipLaunchKernelGGL(eval_bgr8_kernel<3>, dim3(blocks), dim3(EV_THREADS), 0, s, a, groups, (int)vec); break;
    default: hipLaunchKernelGGL(eval_bgr8_kernel<4>, dim3(blocks), dim3(EV_THREADS), 0, s, a, groups, (int)vec); break;
  }
  return hipGetLastError();
}

hipError_t lr_launch_eval_metrics(EvalArgs a, bool fit_gain, bool ssim, void* scratch, hipStream_t s) {
  const uint32_t nblk = (uint32_t)ev_gain_blocks(a.H, a.W);
  const uint32_t blocks = (uint32_t)ev_metric_blocks(a.C, a.H, a.W);
  a.gain_partial = reinterpret_cast<double*>(scratch);
  a.partial = a.gain_partial + 2 * (size_t)a.C * nblk;
  a.ntx = (a.W + EV_T - 1) / EV_T;
  if (fit_gain) {
    if (nblk) hipLaunchKernelGGL(eval_gain_kernel, dim3(nblk * (uint32_t)a.C), dim3(EV_THREADS), 0, s, a, nblk);
    hipLaunchKernelGGL(eval_gain_reduce_kernel, dim3(1), dim3(EV_RED_THREADS), 0, s, (const double*)a.gain_partial, (int)a.C, nblk, a.record);
  }
  if (ssim && fit_gain) hipLaunchKernelGGL((eval_metrics_kernel<true, true>), dim3(blocks), dim3(EV_THREADS), 0, s, a);
  else if (ssim) hipLaunchKernelGGL((eval_metrics_kernel<true, false>), dim3(blocks), dim3(EV_THREADS), 0, s, a);
  else if (fit_gain) hipLaunchKernelGGL((eval_metrics_kernel<false, true>), dim3(blocks), dim3(EV_THREADS), 0, s, a);
  else hipLaunchKernelGGL((eval_metrics_kernel<false, false>), dim3(blocks), dim3(EV_THREADS), 0, s, a);
  const double count = (double)a.C * (double)a.H * (double)a.W;
  hipLaunchKernelGGL(eval_metrics_reduce_kernel, dim3(1), dim3(EV_RED_THREADS), 0, s, (const double*)a.partial, blocks, (int)a.C, count,
                     (int)fit_gain, a.record);
  return hipGetLastError();
}
