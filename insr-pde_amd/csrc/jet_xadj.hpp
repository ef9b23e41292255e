// jet_xadj.hpp -- the adjoint of the sample coordinates of a reverse jet (instantiated by
// jet_xadj.hip; C ABI insr_siren_jet_bwd_x, include/insr_siren.h).
//
// All x-dependence of a jet enters through the first layer's VALUE stream z_0 = W_0 x + b_0: its
// tangent streams are the columns of W_0 and its Laplacian stream is 0, whatever x is (jet_common.hpp
// l0_stream rebuilds them for that reason).  So, for every jet mode,
//     xb[p][k] = sum_m W_0[m][k] zb_0,value[p][m]
// with zb_0,value the value-stream adjoint at layer 0 after the full reverse sweep over all S streams
// (the sine reverse of jet_common.hpp couples the streams per point and neuron, so the tangent and
// Laplacian adjoints reach it: the Hessian-type term of a gradient adjoint, the third-derivative term
// of a Laplacian adjoint).
//
// jet_bwd_x is the propagation half of the tile-split backward (jet_split.hpp jet_bwd_split) at one
// 16-point tile per block, without anything of dW: no h planes, no partial rows, no sums launch.  The
// waves split the neurons of every layer as there (SplitGeo); per layer: sine reverse in registers ->
// the zb planes of all S streams into LDS, point-major [s][16][W + 8] -> barrier -> h-adjoints of the
// layer below, W_j^T zb on v_mfma_f32_16x16x4_f32 with one accumulator per stream.  At layer 0 each lane
// sums its four rows of W_0[:, k] zb, the four lane groups of a point combine by two lane exchanges and
// the waves through a small LDS array in wave order: the result is bit-reproducible.  Exact fp32
// whatever precision the forward ran at (the saved streams are fp32 in one layout for all of them).
#pragma once
#include "jet_split.hpp"

namespace insr {

template <int NT, int S>
constexpr size_t bwd_x_lds_bytes() {
  return (size_t)S * SplitGeo<NT>::PLANE * sizeof(float);
}

// sin/cos of omega * z_layer (value stream) for this wave's rows of one tile: one uniform fast / ocml
// decision for the wave (jet_bwd_split's load_sc at T = 1)
template <int NT, int RPW>
__device__ __forceinline__ void xadj_load_sc(const float* base, int rt0, int lane, floatx4 (&s_)[RPW],
                                             floatx4 (&c_)[RPW]) {
  floatx4 z[RPW];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    z[i] = *reinterpret_cast<const floatx4*>(base + ((rt0 + i) * 64 + lane) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(OMEGA * z[i][r]));
  }
  const bool big = wave_any_big(amax);
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sv, cv;
      if (big)
        sincosf(OMEGA * z[i][r], &sv, &cv);
      else
        sincos_fast(OMEGA * z[i][r], sv, cv);
      s_[i][r] = sv;
      c_[i][r] = cv;
    }
}

template <int NT, int S, bool LAP>
__global__ __launch_bounds__(SplitGeo<NT>::THREADS) void jet_bwd_x(
    int N, int din, int dout, int L, const float* __restrict__ prm, const float* __restrict__ act,
    const float* __restrict__ gy, const float* __restrict__ gdy, const float* __restrict__ glap,
    float* __restrict__ gx) {
  using G = SplitGeo<NT>;
  constexpr int W = G::W, RPW = G::RPW, LDH = G::LDH, PLANE = G::PLANE, WV = G::WV;
  constexpr int NTAN = LAP ? S - 2 : S - 1;
  static_assert(WV * 3 * 16 <= PLANE, "the waves' x-adjoint slots fit the first zb plane");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* zbp = lds;  // zb of layer j, [s][16 points][LDH]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int ntiles = ((N + 63) / 64) * 4;
  const int tile = blockIdx.x;  // < ceil(N / 16): the forward wrote this tile's streams
  const int rt0 = wave * RPW;
  const int p = tile * 16 + c;
  const bool valid = p < N;

  float ga[S][3];
#pragma unroll
  for (int s = 0; s < S; ++s)
    for (int o = 0; o < 3; ++o) ga[s][o] = 0.f;
  if (valid) {
    for (int o = 0; o < dout; ++o) {
      if (gy) ga[0][o] = gy[(long)p * dout + o];
      if (gdy)
        for (int k = 0; k < NTAN; ++k) ga[1 + k][o] = gdy[((long)p * dout + o) * din + k];
      if constexpr (LAP) {
        if (glap) ga[S - 1][o] = glap[(long)p * dout + o];
      }
    }
  }

  // ---- output layer: the seed hb_L = W_out^T g over the d_out outputs (fp32 VALU) ----
  floatx4 sn[RPW], cs[RPW];
  xadj_load_sc<NT, RPW>(act_base(act, L, ntiles, tile, S, NT), rt0, lane, sn, cs);
  const float* Wo = prm + out_off(din, W, L);
  floatx4 hb[RPW][S];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int s = 0; s < S; ++s) hb[i][s] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int o = 0; o < dout; ++o) {
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const floatx4 w4 = *reinterpret_cast<const floatx4*>(Wo + (o * W + 16 * (rt0 + i) + 4 * g));
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) hb[i][s][r] = fmaf(w4[r], ga[s][o], hb[i][s][r]);
    }
  }

  // ---- sine layers j = L .. 0 ----
  for (int j = L; j >= 0; --j) {
    const float* basej = act_base(act, j, ntiles, tile, S, NT);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      floatx4 zs[S];
      zs[0] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 1; s < S; ++s) zs[s] = load_zs<NT, S, LAP>(basej, s, rt0 + i, lane, l0_rebuilt(j, L), prm, din);
      sine_rev<S, LAP>(hb[i], zs, sn[i], cs[i]);
    }
    if (j == 0) break;
    // sin/cos of z_{j-1} for the next sine reverse: their loads fly over the LDS exchange below
    floatx4 snp[RPW], csp[RPW];
    xadj_load_sc<NT, RPW>(act_base(act, j - 1, ntiles, tile, S, NT), rt0, lane, snp, csp);
    __syncthreads();  // the previous layer's LDS readers are done
#pragma unroll
    for (int i = 0; i < RPW; ++i)
#pragma unroll
      for (int s = 0; s < S; ++s)
        *reinterpret_cast<floatx4*>(zbp + s * PLANE + c * LDH + 16 * (rt0 + i) + 4 * g) = hb[i][s];
    __syncthreads();
    {  // propagate: hb_{j-1}[m] (this wave's rows) = sum_n W_j[n][m] zb[n]; A = W^T from L2
      const float* Wj = prm + hidden_off(din, W, j);
      floatx4 nh[RPW][S];
#pragma unroll
      for (int i = 0; i < RPW; ++i)
#pragma unroll
        for (int s = 0; s < S; ++s) nh[i][s] = floatx4{0.f, 0.f, 0.f, 0.f};
      constexpr int KU = NT > 8 ? 2 : NT;  // bounded unroll: W^T loads in flight
#pragma unroll KU
      for (int kt = 0; kt < NT; ++kt) {
        floatx4 wa[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) wa[i][r] = Wj[(16 * kt + 4 * g + r) * W + 16 * (rt0 + i) + c];
        floatx4 b4[S];
#pragma unroll
        for (int s = 0; s < S; ++s)
          b4[s] = *reinterpret_cast<const floatx4*>(zbp + s * PLANE + c * LDH + 16 * kt + 4 * g);
        // r outer: S (x RPW) independent accumulators between dependent MFMAs
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = 0; s < S; ++s)
#pragma unroll
            for (int i = 0; i < RPW; ++i) nh[i][s] = mfma4(wa[i][r], b4[s][r], nh[i][s]);
      }
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        sn[i] = snp[i];
        cs[i] = csp[i];
#pragma unroll
        for (int s = 0; s < S; ++s) hb[i][s] = nh[i][s];
      }
    }
  }

  // ---- layer 0: xb[p][k] = sum_m W_0[m][k] zb_0,value[p][m] ----
  // this lane's rows, then the four lane groups of point c, then the waves in wave order
  float xk[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * (rt0 + i) + 4 * g + r;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < din) xk[k] = fmaf(prm[m * din + k], hb[i][0][r], xk[k]);
    }
  __syncthreads();  // the last propagation's LDS readers are done: the planes are dead
  float* red = lds;  // [WV][3][16]
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = xk[k];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (g == 0) red[(wave * 3 + k) * 16 + c] = v;
  }
  __syncthreads();
  if (wave == 0 && g == 0 && valid) {  // rows past N are never written
    float tot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tot[k] = 0.f;
#pragma unroll
      for (int w = 0; w < WV; ++w) tot[k] += red[(w * 3 + k) * 16 + c];
    }
    float* row = gx + (long)p * din;
    if (din == 1) {
      row[0] = tot[0];
    } else if (din == 2) {
      *reinterpret_cast<float2*>(row) = float2{tot[0], tot[1]};  // (n, 2) rows are 8-B aligned
    } else {
      row[0] = tot[0];
      row[1] = tot[1];
      row[2] = tot[2];
    }
  }
}

template <int NT, int S, bool LAP>
int launch_bwd_x(int N, int din, int dout, int L, const float* prm, const float* act, const float* gy,
                 const float* gdy, const float* glap, float* gx, hipStream_t st) {
  constexpr size_t lds = bwd_x_lds_bytes<NT, S>();
  static_assert(lds <= kLdsMax, "the zb planes fit a CU's LDS");
  const int nb = (N + 15) / 16;
  static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_bwd_x<NT, S, LAP>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
  (void)attr_set;
  hipLaunchKernelGGL((jet_bwd_x<NT, S, LAP>), dim3(nb), dim3(SplitGeo<NT>::THREADS), lds, st, N, din, dout, L, prm,
                     act, gy, gdy, glap, gx);
  return (int)hipGetLastError();
}

}  // namespace insr
