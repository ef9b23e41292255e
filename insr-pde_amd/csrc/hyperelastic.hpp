// hyperelastic.hpp -- per-point hyperelastic materials of the elasticity energy, no SVD.
//
// F = G + I is the deformation gradient, G = df/dx the network's Jacobian (D x D, row-major).
// Both materials are polynomials in F (plus one log) with a closed-form first Piola stress:
//   stable Neo-Hookean (Smith et al. 2018, shifted to zero at rest), c = D / (D + 1):
//     psi = mu/2 (I_C - D) + lam/2 (J - alpha)^2 - mu/2 log(I_C + 1) - psi_0,
//     alpha = 1 + (mu / lam) c,  P = mu (1 - 1 / (I_C + 1)) F + lam (J - alpha) cof F
//   St. Venant-Kirchhoff: E = (F^T F - I) / 2, psi = mu |E|^2 + lam/2 tr(E)^2,
//     P = F (2 mu E + lam tr(E) I)
// Near rest psi is second order in G while its pieces are first order, so everything is
// evaluated from G (the identity never enters a sum that then cancels it):
//   u = I_C - D = |G|^2 + 2 tr G
//   J - 1 = tr G + principal 2x2 minors of G (+ det G when D = 3)
//   cof F = I + C,  C = tr(G) I - G^T (+ cof G when D = 3)
//   psi_NH = mu/2 u + lam/2 (J - 1)(J + 1 - 2 alpha) - mu/2 log1p(u / (D + 1))
//   P_NH   = mu c (G - C) + mu u / ((u + D + 1)(D + 1)) F + lam (J - 1) (I + C)
//   E = (G + G^T + G^T G) / 2,  P_StVK = S + G S
// At G = 0 both values and both stresses are exactly 0.
#pragma once
#include <math.h>

#ifndef INSR_HD
#ifdef __HIPCC__
#define INSR_HD __host__ __device__ __forceinline__
#else
#define INSR_HD inline
#endif
#endif

namespace insr {

// u = I_C - D, jm1 = det F - 1, C = cof F - I
template <int D>
INSR_HD void hyper_geometry(const float (&G)[D * D], float& u, float& jm1, float (&C)[D * D]) {
  float nn = 0.f, tr = 0.f;
#pragma unroll
  for (int k = 0; k < D * D; ++k) nn = fmaf(G[k], G[k], nn);
#pragma unroll
  for (int i = 0; i < D; ++i) tr += G[i * D + i];
  u = nn + 2.f * tr;
  if constexpr (D == 2) {
    jm1 = tr + (G[0] * G[3] - G[1] * G[2]);
    C[0] = G[3];
    C[1] = -G[2];
    C[2] = -G[1];
    C[3] = G[0];
  } else {
    float cg[9];  // cof G
    cg[0] = G[4] * G[8] - G[5] * G[7];
    cg[1] = G[5] * G[6] - G[3] * G[8];
    cg[2] = G[3] * G[7] - G[4] * G[6];
    cg[3] = G[2] * G[7] - G[1] * G[8];
    cg[4] = G[0] * G[8] - G[2] * G[6];
    cg[5] = G[1] * G[6] - G[0] * G[7];
    cg[6] = G[1] * G[5] - G[2] * G[4];
    cg[7] = G[2] * G[3] - G[0] * G[5];
    cg[8] = G[0] * G[4] - G[1] * G[3];
    const float det = G[0] * cg[0] + G[1] * cg[1] + G[2] * cg[2];
    jm1 = tr + (cg[0] + cg[4] + cg[8]) + det;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) C[r * 3 + c] = (r == c ? tr : 0.f) - G[c * 3 + r] + cg[r * 3 + c];
  }
}

// stable Neo-Hookean: returns psi, adds w * dpsi/dF to P (lam > 0)
template <int D>
INSR_HD float neohookean_point(const float (&G)[D * D], float mu, float lam, float w, float (&P)[D * D]) {
  constexpr float c = (float)D / (float)(D + 1);
  float u, jm1, C[D * D];
  hyper_geometry<D>(G, u, jm1, C);
  const float muc = mu * c;
  // (J - alpha)^2 - (1 - alpha)^2 = (J - 1)(J + 1 - 2 alpha), J + 1 - 2 alpha = (J - 1) - 2 (mu / lam) c
  const float psi = 0.5f * mu * u + 0.5f * lam * (jm1 * (jm1 - 2.f * (mu / lam) * c)) - 0.5f * mu * log1pf(u / (D + 1));
  const float a = mu * u / ((u + (D + 1)) * (D + 1)), lj = lam * jm1;
#pragma unroll
  for (int k = 0; k < D * D; ++k) {
    const float id = (k % (D + 1) == 0) ? 1.f : 0.f;
    P[k] += w * (muc * (G[k] - C[k]) + a * (G[k] + id) + lj * (id + C[k]));
  }
  return psi;
}

// St. Venant-Kirchhoff: returns psi, adds w * dpsi/dF to P
template <int D>
INSR_HD float stvk_point(const float (&G)[D * D], float mu, float lam, float w, float (&P)[D * D]) {
  float S[D * D], tr = 0.f, ee = 0.f;  // E, then S = 2 mu E + lam tr(E) I
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      float g = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) g = fmaf(G[k * D + i], G[k * D + j], g);
      const float e = 0.5f * (G[i * D + j] + G[j * D + i] + g);
      S[i * D + j] = e;
      ee = fmaf(e, e, ee);
      if (i == j) tr += e;
    }
  const float psi = mu * ee + 0.5f * lam * (tr * tr);
#pragma unroll
  for (int k = 0; k < D * D; ++k) S[k] = 2.f * mu * S[k] + ((k % (D + 1) == 0) ? lam * tr : 0.f);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      float gs = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) gs = fmaf(G[i * D + k], S[k * D + j], gs);
      P[i * D + j] += w * (S[i * D + j] + gs);
    }
  return psi;
}

}  // namespace insr
