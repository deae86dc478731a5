// Real spherical-harmonics basis shared by the NeRF-SH shading kernels and the octree renderer.
#pragma once
#include <hip/hip_runtime.h>

namespace pxo {

// ------------------------------------------------------------------------------------------
// SH basis (nerf_sh/nerf/sh.py:24-52, :72-108): multipliers of sh[..., k]
// ------------------------------------------------------------------------------------------
template <int DEG>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float (&Y)[(DEG + 1) * (DEG + 1)]) {
  Y[0] = 0.28209479177387814f;
  if constexpr (DEG > 0) {
    Y[1] = -0.4886025119029199f * y;
    Y[2] = 0.4886025119029199f * z;
    Y[3] = -0.4886025119029199f * x;
  }
  if constexpr (DEG > 1) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    Y[4] = 1.0925484305920792f * xy;
    Y[5] = -1.0925484305920792f * yz;
    Y[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
    Y[7] = -1.0925484305920792f * xz;
    Y[8] = 0.5462742152960396f * (xx - yy);
    if constexpr (DEG > 2) {
      Y[9] = -0.5900435899266435f * y * (3.f * xx - yy);
      Y[10] = 2.890611442640554f * xy * z;
      Y[11] = -0.4570457994644658f * y * (4.f * zz - xx - yy);
      Y[12] = 0.3731763325901154f * z * (2.f * zz - 3.f * xx - 3.f * yy);
      Y[13] = -0.4570457994644658f * x * (4.f * zz - xx - yy);
      Y[14] = 1.445305721320277f * z * (xx - yy);
      Y[15] = -0.5900435899266435f * x * (xx - 3.f * yy);
    }
    if constexpr (DEG > 3) {
      Y[16] = 2.5033429417967046f * xy * (xx - yy);
      Y[17] = -1.7701307697799304f * yz * (3.f * xx - yy);
      Y[18] = 0.9461746957575601f * xy * (7.f * zz - 1.f);
      Y[19] = -0.6690465435572892f * yz * (7.f * zz - 3.f);
      Y[20] = 0.10578554691520431f * (zz * (35.f * zz - 30.f) + 3.f);
      Y[21] = -0.6690465435572892f * xz * (7.f * zz - 3.f);
      Y[22] = 0.47308734787878004f * (xx - yy) * (7.f * zz - 1.f);
      Y[23] = -1.7701307697799304f * xz * (xx - 3.f * yy);
      Y[24] = 0.6258357354491761f * (xx * (xx - 3.f * yy) - yy * (3.f * xx - yy));
    }
  }
}

// ------------------------------------------------------------------------------------------
// The basis of a PlenOctree's leaves by run-time width, as the octree renderers and pxo_shade_points evaluate it (both are
// compiled with -ffp-contract=off, so one definition gives one result)
// ------------------------------------------------------------------------------------------
// first `basis_dim` SH basis values (the bands of a lower degree are a prefix of the degree-4 list)
__device__ __forceinline__ void sh_basis_dyn(int basis_dim, float x, float y, float z, float* Y) {
  float tmp[25];
  sh_basis<4>(x, y, z, tmp);
#pragma unroll
  for (int i = 0; i < 25; ++i)
    if (i < basis_dim) Y[i] = tmp[i];
}

// spherical-Gaussian basis of an SG<K> tree (nerf_sh/nerf/sg.py:35-66, svox data_format SG<K>): lobes [K,4] rows
// (lambda, mu.x, mu.y, mu.z), basis_i = exp(lambda_i (mu_i . d - 1)) / K -- float32, evaluated in exactly that order
__device__ __forceinline__ void sg_basis_dyn(int basis_dim, const float* __restrict__ lobes, float x, float y, float z, float* Y) {
  const float inv_k = 1.0f / (float)basis_dim;
  for (int i = 0; i < basis_dim; ++i) {
    const float lam = lobes[4 * i], dot = lobes[4 * i + 1] * x + lobes[4 * i + 2] * y + lobes[4 * i + 3] * z;
    Y[i] = expf(lam * (dot - 1.0f)) * inv_k;
  }
}

}  // namespace pxo
