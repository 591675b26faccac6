// init.hip -- the initialisation pass: LoG.init (/root/reference/LoG/model/level_of_gaussian.py:328-332) with
// Gaussian.init_radius3d (:55-63) over ALL points, for V cameras in one launch.
//
// The reference, per view: exp over [P, 3], normalize over [P, 4], compute_radius, then four boolean-mask reads and
// writes (radius3d[valid] *= 3 / radius2d[valid]; radius3d_min[valid] = minimum(radius3d_min[valid], radius3d[valid])) --
// some fifteen launches and several host synchronisations for 44 bytes read and one float updated per point.
//
// Here a point is one thread's: its activated scale, its normalised quaternion and its world-space covariance do not
// depend on the camera, so they are computed once (the op sequences of the level-of-detail kernel: lod.hip,
// oracle: ora_lod_radius), and the cameras are a loop around the second half of lr_radius_one with the running minimum in
// a register.  No atomics, no LDS; 48 bytes read and at most 4 written per point, whatever V is.  The camera table is
// addressed by the loop counter alone (uniform: scalar loads).
#include "common.hpp"
#include "launch.hpp"

// camera v: cameras[36 v + ...] = proj[16], view[16], fx, fy, tanfovx, tanfovy
#define INIT_CAM_FLOATS 36

__global__ void __launch_bounds__(256)
init_radius3d_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scaling,
                     const float* __restrict__ rotation, int V, const float* __restrict__ cameras,
                     float* __restrict__ radius3d_min, uint8_t* __restrict__ valid_out, float* __restrict__ radius3d_out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
    // every input byte of the row is requested up front
    const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    const float raw[3] = {scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2]};
    const float4 q4 = reinterpret_cast<const float4*>(rotation)[i];
    float m = radius3d_min ? radius3d_min[i] : 0.f;
    const float s[3] = {lr_exp_any(raw[0]), lr_exp_any(raw[1]), lr_exp_any(raw[2])};
    float q[4] = {q4.x, q4.y, q4.z, q4.w};
    lr_normalize4(q);
    float R[9], Sg[6];
    lr_cov3d(s, q, R, Sg);
    bool changed = false, valid = false;
    float r3d = s[0];
    for (int v = 0; v < V; v++) {
      const float* __restrict__ cam = cameras + (size_t)v * INIT_CAM_FLOATS;
      float r = 0.f;
      if (lr_radius_in_ndc(p, cam)) r = lr_radius_of_cov(p, Sg, cam + 16, cam[32], cam[33], cam[34], cam[35]);
      valid = r > 0.f;
      if (valid) {
        const float t = 3.f / r;
        r3d = s[0] * t;
        // torch.minimum: a NaN on either side stays (a NaN m fails the comparison and is kept)
        if (r3d < m || r3d != r3d) { m = r3d; changed = true; }
      }
    }
    if (radius3d_min && changed) radius3d_min[i] = m;
    // the V == 1 form (the launcher's caller has checked it): Gaussian.init_radius3d's own results
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    if (radius3d_out) radius3d_out[i] = valid ? r3d : s[0];
  }
}

// The launch decision: one point per thread, grid-stride, at most 8 workgroups of 256 for each of the 256 CUs (a
// streaming kernel at V = 1 and arithmetic at large V: both want every CU's wave slots filled and nothing queued).
static inline int init_grid(int P) {
  const int blocks = (P + 255) / 256;
  return blocks < 2048 ? blocks : 2048;
}

hipError_t lr_launch_init_radius3d(int P, const float* xyz, const float* scaling, const float* rotation, int V,
                                   const float* cameras, float* radius3d_min, uint8_t* valid, float* radius3d,
                                   hipStream_t s) {
  if (P <= 0) return hipSuccess;
  hipLaunchKernelGGL(init_radius3d_kernel, dim3(init_grid(P)), dim3(256), 0, s, P, xyz, scaling, rotation, V, cameras,
                     radius3d_min, valid, radius3d);
  return hipGetLastError();
}
