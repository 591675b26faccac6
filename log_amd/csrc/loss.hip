// loss.hip -- the photometric training loss of LoG (LoG/render/renderer.py:253-266, LoG/render/loss.py:6-44):
//   loss = a * (1 - mean(ssim_map(render, gt))) + b * mean|render_l1 - gt|,  11x11 Gaussian window (sigma 1.5), no padding.
// The reference runs five grouped conv2d, ~10 element-wise kernels, two reductions and the autograd backward of all of
// them; here: one forward kernel + a one-block fixed-order reduction, and one backward kernel.
//
// Tiling.  A workgroup of 256 threads (4 waves) owns a LS_T x LS_T = 32 x 32 tile of one (b, c) plane.
//   forward : stages the (32+10)^2 input tile of render and gt in LDS, runs the horizontal 11-tap pass for the five
//             moments (42 rows x 32 columns) into LDS, then the vertical pass with four consecutive output rows per
//             thread (14 LDS reads feed 4 x 11 taps), evaluates the SSIM map and leaves three derivative maps.
//   backward: the transposed problem -- a 32 x 32 tile of IMAGE pixels needs the (32+10)^2 tile of the three maps
//             that ends at it; same two passes, then the per-pixel combination with render and gt.
// LDS banking: in every pass the 32 lanes of a half-wave read 32 consecutive elements of one LDS row -- 4-byte elements
// (ds_read_b32: bank (addr/4) % 32 per 32-lane half) or 8-byte pairs (ds_read_b64: bank (addr/4) % 64, 32 lanes x 2
// banks) -- so no pass is strided across rows and no row padding is needed; forward 35.6 KiB (e12 of the horizontal pass
// goes over the consumed input tile), backward 36.4 KiB per workgroup: 4 workgroups per CU of 160 KiB.
//
// Centring.  All moments are taken of (x - 0.5): mu' = w*(x-0.5), s11 = w*(x-0.5)^2 - mu'^2 -- the same real numbers as
// w*x^2 - mu^2 (the window sums to 1) with the cancellation moved from |x|^2 to |x-0.5|^2 (colours live around [0,1]).
// The maps the forward leaves are, per output pixel q and scaled by -a/count (d(loss)/d(ssim_map(q))):
//   maps[0] = d ssim / d mu1' at fixed centred second moments, maps[1] = d ssim / d s11, maps[2] = d ssim / d s12,
// and the backward is  dL/drender(p) = g * sum_q w(p-q) * (maps0(q) + 2 (render(p)-0.5) maps1(q) + (gt(p)-0.5) maps2(q)).
//
// Gain.  The <true> instantiations of the two kernels (lograst_loss_*_gain) take the L1 term of gain[b, c] * render instead
// of a second image: LoG's view correction (renderer.py:243-245) without its render_correct tensor.  The product is one
// fp32 multiply and the subtraction of gt a separate operation (the library is built without contraction), so that
// sign(0) = 0 falls on the pixels where gt == fp32(gain * render), as in the reference.  The backward leaves ONE image
// gradient and, per workgroup, the double sum of sign * render, which loss_gain_reduce_kernel adds per (b, c) in a fixed
// order.  The <false> instantiations are the kernels as they were.
//
// Masks.  The second template flag (lograst_loss_*_masked) takes LoG's mask_ignore blend and MaskForeground's composite
// (renderer.py:255, :356) into the staging of the tile: g = gt * f + (1 - f) * bg[c], x = g * m + render * (1 - m), one fp32
// operation each in the order of the torch expressions, so the results carry the bits of the torch code around the unmasked
// kernels.  The moments are those of (x, g); the L1 term reads x, or render_l1 / gain * render unblended, as the reference's
// render_correct is; the pixel's owner writes g (gt_out), which is the gt of the backward; the backward recomputes x and
// scales what x receives by (1 - m).  In the forward either mask may be NULL (uniform per launch); the masked backward
// always has the ignore mask.  Everything of it stands behind
// `if constexpr (MASKED)`: the <.., false> instantiations are the kernels as they were.
//
// Determinism: fixed tap order (ascending tap index, horizontal then vertical), explicit fmaf only, per-workgroup
// partial sums reduced in a fixed order by one workgroup in double -- no floating-point atomics anywhere.
#include "common.hpp"
#include "launch.hpp"

#define LS_T 32
#define LS_HALO 10
#define LS_IN (LS_T + LS_HALO)
#define LS_THREADS 256
#define LS_ROWS 4                  // consecutive rows per thread in the vertical pass: LS_T * LS_T / LS_ROWS threads
#define LS_CENTER 0.5f
#define LS_STAGE ((LS_IN * LS_IN + LS_THREADS - 1) / LS_THREADS)    // tile elements per thread (7)
#define LS_HITEMS ((LS_IN * LS_T + LS_THREADS - 1) / LS_THREADS)    // horizontal-pass items per thread (6)

// the backward with gain: one double per workgroup of IMAGE tiles -- never fewer than the forward's output tiles, so one
// size serves both launches
size_t lr_loss_gain_scratch_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H < LS_WIN_TAPS || W < LS_WIN_TAPS) return 256;
  const size_t ntx = (size_t)(W + LS_T - 1) / LS_T, nty = (size_t)(H + LS_T - 1) / LS_T;
  const size_t bytes = 8 * ntx * nty * (size_t)B * (size_t)C;
  return (bytes + 255) & ~(size_t)255;
}

size_t lr_loss_scratch_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H < LS_WIN_TAPS || W < LS_WIN_TAPS) return 256;
  const size_t ntx = (size_t)(W - LS_HALO + LS_T - 1) / LS_T, nty = (size_t)(H - LS_HALO + LS_T - 1) / LS_T;
  const size_t bytes = 8 * ntx * nty * (size_t)B * (size_t)C;       // (sum ssim_map, sum |render_l1 - gt|) per workgroup
  return (bytes + 255) & ~(size_t)255;
}

// A (b, c) plane starts at a 64-bit offset (uniform per workgroup); inside it y * stride_y + x * stride_x fits 32 bits
// (checked by the entry points).
LR_DEV const float* ls_plane(const float* p, const int64_t* s, int b, int c) { return p + ((int64_t)b * s[0] + (int64_t)c * s[1]); }

// sum over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; result valid in thread 0
LR_DEV float ls_block_sum(float v, float* ws) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}
// the same in double (the gain gradient's partial sums)
LR_DEV double ls_block_sum(double v, double* ws) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// The moments travel in pairs -- (render, gt), (mu1, mu2), (e11, e22) -- one 8-byte LDS access and one packed fp32
// instruction (v_pk_fma_f32 / v_pk_mul_f32) per pair; element for element the same IEEE operations as scalar code.
template <bool GAIN, bool MASKED>
__global__ void __launch_bounds__(LS_THREADS)
loss_fwd_kernel(LossArgs a) {
  __shared__ lr_f2 srg[LS_IN * LS_IN];                      // (render - 0.5, gt - 0.5)
  __shared__ lr_f2 hmu[LS_IN * LS_T], hee[LS_IN * LS_T];    // horizontal pass: (mu1, mu2), (e11, e22)
  float* he12 = reinterpret_cast<float*>(srg);              // ... and e12, over the input tile once it has been consumed
  float* ws = he12 + LS_IN * LS_T;                          // 8 floats for the two workgroup sums (35.6 KiB in all: 4 per CU)
  const int tid = (int)threadIdx.x;
  int t = (int)blockIdx.x;
  const int c = t % a.C; t /= a.C;
  const int tx = t % a.ntx; t /= a.ntx;
  const int ty = t % a.nty;
  const int b = t / a.nty;
  const int x0 = tx * LS_T, y0 = ty * LS_T;
  const bool last_x = tx == a.ntx - 1, last_y = ty == a.nty - 1;
  const int OW = a.W - LS_HALO, OH = a.H - LS_HALO;
  const float* rp = ls_plane(a.render, a.rs, b, c);
  const float* gp = ls_plane(a.gt, a.gs, b, c);
  const float* lp = (!GAIN && a.render_l1) ? ls_plane(a.render_l1, a.ls, b, c) : nullptr;
  const int rsy = (int)a.rs[2], rsx = (int)a.rs[3], gsy = (int)a.gs[2], gsx = (int)a.gs[3], lsy = (int)a.ls[2], lsx = (int)a.ls[3];
  float gain = 1.f;
  if constexpr (GAIN) gain = a.gain[b * a.C + c];
  // MASKED: the ignore mask and the foreground mask of image b (either may be NULL: uniform per launch), shared by the
  // C workgroups of a tile, which are adjacent in blockIdx
  const float* mp = nullptr;
  const float* fp = nullptr;
  int msy = 0, msx = 0, fsy = 0, fsx = 0;
  float bgc = 0.f;
  if constexpr (MASKED) {
    if (a.mask) { mp = a.mask + (int64_t)b * a.ms[0]; msy = (int)a.ms[1]; msx = (int)a.ms[2]; }
    if (a.fg) { fp = a.fg + (int64_t)b * a.fs[0]; fsy = (int)a.fs[1]; fsx = (int)a.fs[2]; bgc = a.bg[c]; }
  }

  // stage the input tile: all of a thread's loads are requested before the first is used.  Every image pixel belongs to
  // exactly one tile's L1 sum (the last tile of a row / column also owns its halo).
  float rv[LS_STAGE], gv[LS_STAGE], lv[LS_STAGE];
  [[maybe_unused]] float mv[LS_STAGE], fv[LS_STAGE];        // MASKED only
  bool own[LS_STAGE];
#pragma unroll
  for (int u = 0; u < LS_STAGE; u++) {
    const int i = tid + u * LS_THREADS;
    const int ly = i / LS_IN, lx = i - ly * LS_IN;
    const int y = y0 + ly, x = x0 + lx;
    const bool in = i < LS_IN * LS_IN && y < a.H && x < a.W;
    own[u] = in && (lx < LS_T || last_x) && (ly < LS_T || last_y);
    rv[u] = in ? rp[y * rsy + x * rsx] : LS_CENTER;
    gv[u] = in ? gp[y * gsy + x * gsx] : LS_CENTER;
    lv[u] = (lp && own[u]) ? lp[y * lsy + x * lsx] : 0.f;
    if constexpr (MASKED) {
      mv[u] = (mp && in) ? mp[y * msy + x * msx] : 0.f;
      fv[u] = (fp && in) ? fp[y * fsy + x * fsx] : 1.f;
    }
  }
  float l1 = 0.f;
#pragma unroll
  for (int u = 0; u < LS_STAGE; u++) {
    const int i = tid + u * LS_THREADS;
    if constexpr (MASKED) {
      // gt = gt * f + (1 - f) * bg, then the SSIM input x = gt * m + render * (1 - m): one fp32 operation each, in the
      // order of the reference's torch expressions; out-of-image elements stay LS_CENTER for both
      const int ly = i / LS_IN, lx = i - ly * LS_IN;
      const int y = y0 + ly, x = x0 + lx;
      const bool in = i < LS_IN * LS_IN && y < a.H && x < a.W;
      float g = gv[u], xs = rv[u];
      if (in) {
        if (fp) g = (g * fv[u]) + ((1.f - fv[u]) * bgc);
        if (a.gt_out && own[u]) a.gt_out[(((int64_t)b * a.C + c) * a.H + y) * a.W + x] = g;
        if (mp) xs = (g * mv[u]) + (xs * (1.f - mv[u]));
      }
      if (own[u]) l1 += fabsf((GAIN ? gain * rv[u] : (lp ? lv[u] : xs)) - g);   // gain and render_l1 read the plain render
      if (i < LS_IN * LS_IN) srg[i] = lr_f2{xs - LS_CENTER, g - LS_CENTER};
    } else {
      if constexpr (GAIN) { if (own[u]) l1 += fabsf(gain * rv[u] - gv[u]); }
      else if (own[u]) l1 += fabsf((lp ? lv[u] : rv[u]) - gv[u]);
      if (i < LS_IN * LS_IN) srg[i] = lr_f2{rv[u] - LS_CENTER, gv[u] - LS_CENTER};
    }
  }
  __syncthreads();

  // horizontal pass: 42 rows x 32 columns, five moments
  float e12v[LS_HITEMS];
#pragma unroll
  for (int u = 0; u < LS_HITEMS; u++) {
    const int i = tid + u * LS_THREADS;
    e12v[u] = 0.f;
    if (i < LS_IN * LS_T) {
      const int row = i / LS_T, hx = i - row * LS_T;
      const lr_f2* p = srg + row * LS_IN + hx;
      lr_f2 mu = {0.f, 0.f}, ee = {0.f, 0.f};
      float e12 = 0.f;
#pragma unroll
      for (int k = 0; k < LS_WIN_TAPS; k++) {
        const float w = a.w[k];
        const lr_f2 v = p[k], w2 = {w, w};
        mu = lr_fma2(w2, v, mu);
        ee = lr_fma2(w2, v * v, ee);
        e12 = lr_fma(w, v.x * v.y, e12);
      }
      hmu[i] = mu; hee[i] = ee; e12v[u] = e12;
    }
  }
  __syncthreads();                                          // every read of the input tile is done: e12 goes over it
#pragma unroll
  for (int u = 0; u < LS_HITEMS; u++) {
    const int i = tid + u * LS_THREADS;
    if (i < LS_IN * LS_T) he12[i] = e12v[u];
  }
  __syncthreads();

  // vertical pass: column xo, output rows yq .. yq+3 out of LDS rows yq .. yq+13
  const int xo = tid & (LS_T - 1), yq = (tid / LS_T) * LS_ROWS;
  lr_f2 amu[LS_ROWS], aee[LS_ROWS];
  float a12[LS_ROWS];
#pragma unroll
  for (int j = 0; j < LS_ROWS; j++) { amu[j] = lr_f2{0.f, 0.f}; aee[j] = lr_f2{0.f, 0.f}; a12[j] = 0.f; }
#pragma unroll
  for (int rr = 0; rr < LS_ROWS + LS_HALO; rr++) {
    const int o = (yq + rr) * LS_T + xo;
    const lr_f2 vmu = hmu[o], vee = hee[o];
    const float v12 = he12[o];
#pragma unroll
    for (int j = 0; j < LS_ROWS; j++) {
      const int k = rr - j;
      if (k >= 0 && k < LS_WIN_TAPS) {
        const lr_f2 w2 = {a.w[k], a.w[k]};
        amu[j] = lr_fma2(w2, vmu, amu[j]);
        aee[j] = lr_fma2(w2, vee, aee[j]);
        a12[j] = lr_fma(a.w[k], v12, a12[j]);
      }
    }
  }

  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  float ssum = 0.f;
  const int ox = x0 + xo;
  const int64_t plane = (int64_t)OH * OW, bc = (int64_t)b * a.C + c, nbc = (int64_t)a.B * a.C;
  float* map0 = a.maps + bc * plane;                       // uniform per workgroup
  float* map1 = map0 + nbc * plane;
  float* map2 = map1 + nbc * plane;
#pragma unroll
  for (int j = 0; j < LS_ROWS; j++) {
    const int oy = y0 + yq + j;
    if (ox >= OW || oy >= OH) continue;
    const float m1c = amu[j].x, m2c = amu[j].y;
    const float s11 = aee[j].x - m1c * m1c, s22 = aee[j].y - m2c * m2c, s12 = a12[j] - m1c * m2c;
    const float mu1 = m1c + LS_CENTER, mu2 = m2c + LS_CENTER;
    const float n1 = lr_fma(2.f * mu1, mu2, C1), n2 = lr_fma(2.f, s12, C2);
    const float d1 = lr_fma(mu1, mu1, lr_fma(mu2, mu2, C1)), d2 = (s11 + s22) + C2;
    const float inv = 1.f / (d1 * d2);                      // the one division; 1/d1 = inv * d2, 1/d2 = inv * d1
    const float ssim = (n1 * n2) * inv;
    ssum += ssim;
    if (a.maps) {
      const float id1 = inv * d2, id2 = inv * d1;
      const float ds11 = -(ssim * id2);
      const float ds12 = (2.f * n1) * inv;
      const float t1 = (2.f * mu2) * (n2 * inv) - (2.f * mu1) * (ssim * id1);    // through n1 and d1 only
      const float dm1 = (t1 - (2.f * m1c) * ds11) - m2c * ds12;
      const int o = oy * OW + ox;
      map0[o] = a.scale * dm1;
      map1[o] = a.scale * ds11;
      map2[o] = a.scale * ds12;
    }
  }
  const float bs = ls_block_sum(ssum, ws);
  const float bl = ls_block_sum(l1, ws + 4);
  if (tid == 0) reinterpret_cast<float2*>(a.partial)[blockIdx.x] = make_float2(bs, bl);
}

// one workgroup of 1024: thread t adds partials t, t+1024, ... (four independent chains, combined in order) in double,
// then a fixed tree over the threads
#define LS_RED_THREADS 1024
__global__ void __launch_bounds__(LS_RED_THREADS)
loss_reduce_kernel(const float2* __restrict__ partial, uint32_t n, double inv_count, double inv_count_l1, float wa, float wb,
                   float* __restrict__ out3) {
  __shared__ double s0[LS_RED_THREADS], s1[LS_RED_THREADS];
  double c0[4] = {0.0, 0.0, 0.0, 0.0}, c1[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t base = 0; base < n; base += 4u * LS_RED_THREADS) {
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) {
      const uint32_t i = base + u * LS_RED_THREADS + threadIdx.x;
      if (i < n) {
        const float2 v = partial[i];
        c0[u] += (double)v.x;
        c1[u] += (double)v.y;
      }
    }
  }
  s0[threadIdx.x] = (c0[0] + c0[1]) + (c0[2] + c0[3]);
  s1[threadIdx.x] = (c1[0] + c1[1]) + (c1[2] + c1[3]);
  __syncthreads();
  for (uint32_t d = LS_RED_THREADS / 2; d >= 1; d >>= 1) {
    if (threadIdx.x < d) { s0[threadIdx.x] += s0[threadIdx.x + d]; s1[threadIdx.x] += s1[threadIdx.x + d]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double ssim = 1.0 - s0[0] * inv_count, l1 = s1[0] * inv_count_l1;
    out3[0] = (float)((double)wa * ssim + (double)wb * l1);
    out3[1] = (float)l1;
    out3[2] = (float)ssim;
  }
}

// one workgroup per (b, c): thread t adds the plane's partials t, t + 256, ... in double, then a fixed tree over the threads;
// grad_gain[b, c] = gl * l1_scale * sum, rounded to fp32 once
#define LS_GAIN_RED_THREADS 256
__global__ void __launch_bounds__(LS_GAIN_RED_THREADS)
loss_gain_reduce_kernel(const double* __restrict__ partial, int C, uint32_t tiles, const float* __restrict__ grad_loss, float l1_scale,
                        float* __restrict__ grad_gain) {
  __shared__ double s[LS_GAIN_RED_THREADS];
  const uint32_t b = blockIdx.x / (uint32_t)C, c = blockIdx.x - b * (uint32_t)C;
  const double* p = partial + ((size_t)b * tiles) * (size_t)C + c;      // tile t of the plane: p[t * C]
  double acc = 0.0;
  for (uint32_t t = threadIdx.x; t < tiles; t += LS_GAIN_RED_THREADS) acc += p[(size_t)t * (size_t)C];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t d = LS_GAIN_RED_THREADS / 2; d >= 1; d >>= 1) {
    if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad_gain[blockIdx.x] = (float)(((double)grad_loss[0] * (double)l1_scale) * s[0]);
}

template <bool GAIN, bool MASKED>
__global__ void __launch_bounds__(LS_THREADS)
loss_bwd_kernel(LossArgs a, const float* __restrict__ grad_loss, float* __restrict__ g_render, float* __restrict__ g_render_l1) {
  __shared__ lr_f2 sm01[LS_IN * LS_IN];                     // (maps0, maps1)
  __shared__ float sm2[LS_IN * LS_IN];
  __shared__ lr_f2 hm01[LS_IN * LS_T];
  __shared__ float hm2[LS_IN * LS_T];
  const int tid = (int)threadIdx.x;
  int t = (int)blockIdx.x;
  const int c = t % a.C; t /= a.C;
  const int tx = t % a.ntx; t /= a.ntx;
  const int ty = t % a.nty;
  const int b = t / a.nty;
  const int x0 = tx * LS_T, y0 = ty * LS_T;
  const int OW = a.W - LS_HALO, OH = a.H - LS_HALO;
  const int64_t plane = (int64_t)OH * OW, bc = (int64_t)b * a.C + c, nbc = (int64_t)a.B * a.C;
  const float* map0 = a.maps + bc * plane;                 // uniform per workgroup
  const float* map1 = map0 + nbc * plane;
  const float* map2 = map1 + nbc * plane;

  // the image values of this thread's four pixels are requested first (used last)
  const int xo = tid & (LS_T - 1), yq = (tid / LS_T) * LS_ROWS;
  const int x = x0 + xo;
  const float* rp = ls_plane(a.render, a.rs, b, c);
  const float* gp = ls_plane(a.gt, a.gs, b, c);
  const float* lp = (!GAIN && a.render_l1) ? ls_plane(a.render_l1, a.ls, b, c) : nullptr;
  const int rsy = (int)a.rs[2], rsx = (int)a.rs[3], gsy = (int)a.gs[2], gsx = (int)a.gs[3], lsy = (int)a.ls[2], lsx = (int)a.ls[3];
  float gain = 1.f;
  if constexpr (GAIN) gain = a.gain[b * a.C + c];
  float pr[LS_ROWS], pg[LS_ROWS], pl[LS_ROWS];
  // MASKED only: the ignore mask, never NULL here (a.gt is the composited gt; a composite without a blend takes the
  // unmasked backward on it)
  [[maybe_unused]] float pm[LS_ROWS];
  const float* mp = nullptr;
  int msy = 0, msx = 0;
  if constexpr (MASKED) { mp = a.mask + (int64_t)b * a.ms[0]; msy = (int)a.ms[1]; msx = (int)a.ms[2]; }
#pragma unroll
  for (int j = 0; j < LS_ROWS; j++) {
    const int y = y0 + yq + j;
    const bool in = x < a.W && y < a.H;
    pr[j] = in ? rp[y * rsy + x * rsx] : 0.f;
    pg[j] = in ? gp[y * gsy + x * gsx] : 0.f;
    pl[j] = (in && lp) ? lp[y * lsy + x * lsx] : 0.f;
    if constexpr (MASKED) pm[j] = in ? mp[y * msy + x * msx] : 0.f;
  }

  // maps at q = p - 10 .. p (zero outside the valid region); all loads requested before the first is used
  float v0[LS_STAGE], v1[LS_STAGE], v2[LS_STAGE];
#pragma unroll
  for (int u = 0; u < LS_STAGE; u++) {
    const int i = tid + u * LS_THREADS;
    const int ly = i / LS_IN, lx = i - ly * LS_IN;
    const int qy = y0 - LS_HALO + ly, qx = x0 - LS_HALO + lx;
    const bool in = i < LS_IN * LS_IN && qy >= 0 && qy < OH && qx >= 0 && qx < OW;
    const int o = qy * OW + qx;
    v0[u] = in ? map0[o] : 0.f;
    v1[u] = in ? map1[o] : 0.f;
    v2[u] = in ? map2[o] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < LS_STAGE; u++) {
    const int i = tid + u * LS_THREADS;
    if (i < LS_IN * LS_IN) { sm01[i] = lr_f2{v0[u], v1[u]}; sm2[i] = v2[u]; }
  }
  __syncthreads();

  // horizontal: image column xo gets tap k from map column xo - k (local xo + 10 - k)
  for (int i = tid; i < LS_IN * LS_T; i += LS_THREADS) {
    const int row = i / LS_T, hx = i - row * LS_T;
    const int base = row * LS_IN + hx + LS_HALO;
    lr_f2 h01 = {0.f, 0.f};
    float h2 = 0.f;
#pragma unroll
    for (int k = 0; k < LS_WIN_TAPS; k++) {
      const float w = a.w[k];
      h01 = lr_fma2(lr_f2{w, w}, sm01[base - k], h01);
      h2 = lr_fma(w, sm2[base - k], h2);
    }
    hm01[i] = h01; hm2[i] = h2;
  }
  __syncthreads();

  // vertical: image row yq + j gets tap k from LDS row yq + j + 10 - k; rows walked downwards so that k ascends
  lr_f2 a01[LS_ROWS];
  float a2[LS_ROWS];
#pragma unroll
  for (int j = 0; j < LS_ROWS; j++) { a01[j] = lr_f2{0.f, 0.f}; a2[j] = 0.f; }
#pragma unroll
  for (int rr = LS_ROWS + LS_HALO - 1; rr >= 0; rr--) {
    const int o = (yq + rr) * LS_T + xo;
    const lr_f2 v01 = hm01[o];
    const float v2 = hm2[o];
#pragma unroll
    for (int j = 0; j < LS_ROWS; j++) {
      const int k = j + LS_HALO - rr;
      if (k >= 0 && k < LS_WIN_TAPS) {
        a01[j] = lr_fma2(lr_f2{a.w[k], a.w[k]}, v01, a01[j]);
        a2[j] = lr_fma(a.w[k], v2, a2[j]);
      }
    }
  }

  const float gl = grad_loss[0];
  if constexpr (!GAIN) { if (x >= a.W) return; }                    // (with gain every thread reaches the workgroup sum)
  const int64_t out_plane = bc * ((int64_t)a.H * a.W);
  float sr = 0.f;                                                   // with gain: sum of sign * render over this thread's pixels
#pragma unroll
  for (int j = 0; j < LS_ROWS; j++) {
    const int y = y0 + yq + j;
    if (y >= a.H || (GAIN && x >= a.W)) continue;
    const float r = pr[j], g = pg[j];
    if constexpr (MASKED) {
      // the SSIM input is the blend x (recomputed with the forward's operations); render gets (1 - m) of what x gets,
      // the gain's and render_l1's L1 terms read the plain render and pass unscaled
      const float keep = 1.f - pm[j];
      const float xs = (g * pm[j]) + (r * keep);
      float G = gl * lr_fma(g - LS_CENTER, a2[j], lr_fma(2.f * (xs - LS_CENTER), a01[j].y, a01[j].x));
      const float d = (GAIN ? gain * r : (lp ? pl[j] : xs)) - g;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      const float l1g = gl * (a.l1_scale * sgn);
      const int o = y * a.W + x;
      if constexpr (GAIN) { G = (keep * G) + gain * l1g; sr += sgn * r; }
      else if (lp) { g_render_l1[out_plane + o] = l1g; G = keep * G; }
      else { G += l1g; G = keep * G; }
      g_render[out_plane + o] = G;
    } else {
      float G = gl * lr_fma(g - LS_CENTER, a2[j], lr_fma(2.f * (r - LS_CENTER), a01[j].y, a01[j].x));
      const float d = (GAIN ? gain * r : (lp ? pl[j] : r)) - g;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);       // sign(0) = 0, as torch.nn.L1Loss
      const float l1g = gl * (a.l1_scale * sgn);
      const int o = y * a.W + x;
      if constexpr (GAIN) { G += gain * l1g; sr += sgn * r; }
      else if (lp) g_render_l1[out_plane + o] = l1g;
      else G += l1g;
      g_render[out_plane + o] = G;
    }
  }
  if constexpr (GAIN) {
    __shared__ double gws[4];
    const double bsum = ls_block_sum((double)sr, gws);
    if (tid == 0) a.gain_partial[blockIdx.x] = bsum;
  }
}

// The instantiation follows the arguments: a.gain selects GAIN; a.mask or a.fg selects MASKED in the forward, a.mask in the
// backward (a composite alone leaves its gt_out, and the backward is the unmasked one on it).
hipError_t lr_launch_loss_fwd(const LossArgs& a, float wa, float wb, float* out3, hipStream_t s) {
  const uint32_t blocks = (uint32_t)a.ntx * (uint32_t)a.nty * (uint32_t)a.B * (uint32_t)a.C;
  const bool masked = a.mask || a.fg;
  lr_prof_begin(LRK_LOSS_FWD, s);
  auto kernel = a.gain ? (masked ? loss_fwd_kernel<true, true> : loss_fwd_kernel<true, false>)
                       : (masked ? loss_fwd_kernel<false, true> : loss_fwd_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LS_THREADS), 0, s, a);
  const double count = (double)a.B * a.C * (double)(a.H - LS_HALO) * (double)(a.W - LS_HALO);
  const double count_l1 = (double)a.B * a.C * (double)a.H * (double)a.W;
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(LS_RED_THREADS), 0, s, reinterpret_cast<const float2*>(a.partial), blocks, 1.0 / count,
                     1.0 / count_l1, wa, wb, out3);
  lr_prof_end(LRK_LOSS_FWD, s);
  return hipGetLastError();
}

// g_render_l1 where a.render_l1 is set, grad_gain (the reduction of the workgroups' partial sums) where a.gain is: else NULL
hipError_t lr_launch_loss_bwd(const LossArgs& a, const float* grad_loss, float* g_render, float* g_render_l1, float* grad_gain,
                              hipStream_t s) {
  const uint32_t tiles = (uint32_t)a.ntx * (uint32_t)a.nty, planes = (uint32_t)a.B * (uint32_t)a.C;
  lr_prof_begin(LRK_LOSS_BWD, s);
  auto kernel = a.gain ? (a.mask ? loss_bwd_kernel<true, true> : loss_bwd_kernel<true, false>)
                       : (a.mask ? loss_bwd_kernel<false, true> : loss_bwd_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(tiles * planes), dim3(LS_THREADS), 0, s, a, grad_loss, g_render, g_render_l1);
  if (a.gain)
    hipLaunchKernelGGL(loss_gain_reduce_kernel, dim3(planes), dim3(LS_GAIN_RED_THREADS), 0, s, (const double*)a.gain_partial, (int)a.C,
                       tiles, grad_loss, a.l1_scale, grad_gain);
  lr_prof_end(LRK_LOSS_BWD, s);
  return hipGetLastError();
}

// ---- bounding box of a foreground mask (MaskForeground.bound_from_mask, renderer.py:319-326) ------------------------
// One pass over a strided fp32 mask [B, H, W]: per image the int32 record {xmin, ymin, xmax, ymax, count, 0, 0, 0} of the
// pixels with mask > threshold (strict: a NaN is not foreground).  A workgroup takes MB_ROWS row(s) of one image, lane after
// lane along x (consecutive dwords of a row with stride 1); the five integers are reduced over the wave by shuffles, over
// the four waves through LDS, and one thread commits them with integer atomicMin / atomicMax / atomicAdd: exact and
// independent of the order.
#define MB_THREADS 256
#define MB_ROWS 4                  // rows per workgroup: 270 workgroups at 1080p (one row each: four times the atomics on one
                                   // record, measured twice as slow)
#define MB_UNROLL 4                // loads in flight per thread

__global__ void mask_bounds_init_kernel(int32_t* __restrict__ record, int B, int H, int W) {
  for (int b = (int)threadIdx.x; b < B; b += (int)blockDim.x) {
    int32_t* r = record + (size_t)b * MB_RECORD_INTS;
    r[0] = W; r[1] = H; r[2] = -1; r[3] = -1;
    r[4] = 0; r[5] = 0; r[6] = 0; r[7] = 0;
  }
}

__global__ void __launch_bounds__(MB_THREADS)
mask_bounds_kernel(const float* __restrict__ mask, int64_t sb, int64_t sy, int64_t sx, int H, int W, int strips, float threshold,
                   int32_t* __restrict__ record) {
  __shared__ int32_t red[4][5];
  const int b = (int)(blockIdx.x / (uint32_t)strips), strip = (int)(blockIdx.x - (uint32_t)b * (uint32_t)strips);
  const float* mp = mask + (int64_t)b * sb;
  const int yb = strip * MB_ROWS, ye = min(yb + MB_ROWS, H);
  int xmin = W, ymin = H, xmax = -1, ymax = -1, count = 0;
  for (int y = yb; y < ye; y++) {
    const float* row = mp + (int64_t)y * sy;
    for (int xb = (int)threadIdx.x; xb < W; xb += MB_UNROLL * MB_THREADS) {
      float v[MB_UNROLL];                                           // all of a round's loads are requested before the first is used
#pragma unroll
      for (int u = 0; u < MB_UNROLL; u++) {
        const int x = xb + u * MB_THREADS;
        v[u] = x < W ? row[(int64_t)x * sx] : threshold;            // (threshold > threshold is false)
      }
#pragma unroll
      for (int u = 0; u < MB_UNROLL; u++) {
        const int x = xb + u * MB_THREADS;
        if (v[u] > threshold) {
          xmin = min(xmin, x); xmax = max(xmax, x);
          ymin = min(ymin, y); ymax = max(ymax, y);
          count++;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    xmin = min(xmin, __shfl_down(xmin, d)); ymin = min(ymin, __shfl_down(ymin, d));
    xmax = max(xmax, __shfl_down(xmax, d)); ymax = max(ymax, __shfl_down(ymax, d));
    count += __shfl_down(count, d);
  }
  const int wave = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63u) == 0) { red[wave][0] = xmin; red[wave][1] = ymin; red[wave][2] = xmax; red[wave][3] = ymax; red[wave][4] = count; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; w++) {
      xmin = min(xmin, red[w][0]); ymin = min(ymin, red[w][1]);
      xmax = max(xmax, red[w][2]); ymax = max(ymax, red[w][3]);
      count += red[w][4];
    }
    if (count > 0) {
      // The record only ever tightens, so a bound that an earlier read of it already meets needs no atomic (a stale read
      // costs an atomic, never a result): a box-shaped mask leaves most workgroups the count alone.
      int32_t* r = record + (size_t)b * MB_RECORD_INTS;
      if (xmin < __hip_atomic_load(r + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(r + 0, xmin);
      if (ymin < __hip_atomic_load(r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(r + 1, ymin);
      if (xmax > __hip_atomic_load(r + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(r + 2, xmax);
      if (ymax > __hip_atomic_load(r + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(r + 3, ymax);
      atomicAdd(r + 4, count);
    }
  }
}

hipError_t lr_launch_mask_bounds(int B, int H, int W, const float* mask, const int64_t* ms, float threshold, int32_t* record, hipStream_t s) {
  const int strips = (H + MB_ROWS - 1) / MB_ROWS;
  hipLaunchKernelGGL(mask_bounds_init_kernel, dim3(1), dim3(64), 0, s, record, B, H, W);
  if (strips > 0 && W > 0) hipLaunchKernelGGL(mask_bounds_kernel, dim3((uint32_t)B * (uint32_t)strips), dim3(MB_THREADS), 0, s, mask, ms[0], ms[1], ms[2], H, W, strips,
                     threshold, record);
  return hipGetLastError();
}

// Instantiated here, in the order the code object has had them since each was added: the device code then compares equal
// byte for byte whatever the host code above does.
template __global__ void loss_fwd_kernel<true, false>(LossArgs);
template __global__ void loss_fwd_kernel<false, false>(LossArgs);
template __global__ void loss_bwd_kernel<false, false>(LossArgs, const float*, float*, float*);
template __global__ void loss_bwd_kernel<true, false>(LossArgs, const float*, float*, float*);
template __global__ void loss_fwd_kernel<true, true>(LossArgs);
template __global__ void loss_fwd_kernel<false, true>(LossArgs);
template __global__ void loss_bwd_kernel<true, true>(LossArgs, const float*, float*, float*);
template __global__ void loss_bwd_kernel<false, true>(LossArgs, const float*, float*, float*);
