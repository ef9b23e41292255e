// jet_hess.hpp -- second-order SIREN jets: y, the Jacobian and the FULL Hessian of a d-input
// SIREN (d = 2, 3) in one forward launch, every parameter gradient in one reverse launch
// (instantiated by jet_hess.hip; the C ABI is insr_siren_hess_fwd / insr_siren_hess_bwd).
//
// Math (one more jet family beside jet_common.hpp's).  Per point and neuron the jet carries
//   value z, tangents t_i (i < d), second-order u_ij for the pairs i <= j in row-major
//   upper-triangle order (d = 2: 00 01 11; d = 3: 00 01 02 11 12 22)
// i.e. S = 1 + d + d (d + 1) / 2 streams (6 / 10): stream 0 the value, 1..d the tangents, 1 + d.. the
// pairs.  Linear layers act on every stream with the same W (bias on the value only); the first
// layer gives z = W0 x + b0, t_i = W0[:, i], u_ij = 0 (only its value stream is saved: readers
// rebuild the rest).  The sine couples the streams lane-locally (s, c = sin, cos(w z)):
//   h = s,  dh_i = w c t_i,  hh_ij = w c u_ij - w^2 s t_i t_j
// and its reverse (adjoints hb, dhb_i, hhb_ij, one per pair):
//   zb    = w c hb - w^2 s sum_i t_i dhb_i - sum_{i<=j} hhb_ij (w^2 s u_ij + w^3 c t_i t_j)
//   tb_i  = w c dhb_i - w^2 s sum_j (1 + delta_ij) t_j hhb_{ij}
//   ub_ij = w c hhb_ij
// Weight gradients: dW = sum over streams and points of zb (x) h_prev; the first layer's
// dW0[:, k] = sum_p zb x_k + tb_k (its u streams carry no parameter).
//
// Kernels: the dataflow of the exact-fp32 tile-split pair (jet_split.hpp) at T = 1 -- the waves of a
// block own the 16-row tiles of every layer, one 16-point tile per block, products on
// v_mfma_f32_16x16x4_f32 with independent accumulators, point-major LDS planes [s][16][W + 8]
// for the B operand, the swizzled neuron-major h planes (hT_index) for dW, one wave-uniform
// fast / ocml sin-cos choice.  Exact fp32 whatever the network's precision.
//
// LDS.  The forward holds S planes (S 16 (W + 8) 4 bytes: 87,040 at S = 10, W = 128).  The backward
// needs a zb and an h plane per stream (S (16 (W + 8) + 16 W) 4 bytes: 168,960 at S = 10, W = 128,
// over the 160 KB of a CU), so it stages its streams in NG groups of GS = S / NG: the zb / h planes of
// a group into LDS, barrier, dW += and W^T zb for that group, next group.  dW is a sum over the
// streams and the propagation is independent per stream, so grouping changes no result beyond
// fp32 summation order.
#pragma once
#include "jet_split.hpp"

namespace insr {

template <int D>
struct HessGeo {
  static constexpr int NP = D * (D + 1) / 2;  // unordered pairs i <= j
  static constexpr int S = 1 + D + NP;        // streams
};
// pair p (row-major upper triangle) <-> (i, j), i <= j; d <= 3
template <int D>
__host__ __device__ constexpr int pair_of(int i, int j) { return i * D - i * (i - 1) / 2 + (j - i); }
template <int D>
__host__ __device__ constexpr int pair_row(int p) { return (p >= D ? 1 : 0) + (p >= 2 * D - 1 ? 1 : 0); }
template <int D>
__host__ __device__ constexpr int pair_col(int p) { return p - pair_of<D>(pair_row<D>(p), pair_row<D>(p)) + pair_row<D>(p); }

// streams per LDS group of the backward (all of them where they fit a CU's LDS, else half)
template <int NT, int D>
constexpr int hess_group() {
  constexpr int S = HessGeo<D>::S;
  return (size_t)S * (SplitGeo<NT>::PLANE + 16 * 16 * NT) * sizeof(float) <= kLdsMax ? S : S / 2;
}
template <int NT, int D>
constexpr size_t fwd_hess_lds_bytes() { return (size_t)HessGeo<D>::S * SplitGeo<NT>::PLANE * sizeof(float); }
template <int NT, int D>
constexpr size_t bwd_hess_lds_bytes() {
  return (size_t)hess_group<NT, D>() * (SplitGeo<NT>::PLANE + 16 * 16 * NT) * sizeof(float);
}

// ---- the sine on a second-order jet, one row tile, in place (z-streams in, h-streams out) ----
template <int D, bool FAST>
__device__ __forceinline__ void sine_jet2_impl(floatx4 (&a)[HessGeo<D>::S]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float arg = OMEGA * a[0][r];
    float sn, cs;
    if constexpr (FAST) sincos_fast(arg, sn, cs); else sincosf(arg, &sn, &cs);
    const float wc = OMEGA * cs, ws = OMEGA2 * sn;
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j, ++p) a[1 + D + p][r] = wc * a[1 + D + p][r] - ws * (a[1 + i][r] * a[1 + j][r]);
#pragma unroll
    for (int i = 0; i < D; ++i) a[1 + i][r] *= wc;
    a[0][r] = sn;
  }
}
template <int D>
__device__ __forceinline__ void sine_jet2(floatx4 (&a)[HessGeo<D>::S]) {
  float amax = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(OMEGA * a[0][r]));
  if (wave_any_big(amax))
    sine_jet2_impl<D, false>(a);
  else
    sine_jet2_impl<D, true>(a);
}

// h-stream s of a sine layer from its z-streams (zs[0] unread) and sin / cos of its value stream
template <int D>
__device__ __forceinline__ floatx4 h_stream2(int s, const floatx4 (&zs)[HessGeo<D>::S], const floatx4& sn,
                                             const floatx4& cs) {
  if (s == 0) return sn;
  floatx4 out;
  if (s <= D) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = OMEGA * cs[r] * zs[s][r];
  } else {
    const int p = s - 1 - D, i = pair_row<D>(p), j = pair_col<D>(p);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = OMEGA * cs[r] * zs[s][r] - OMEGA2 * sn[r] * (zs[1 + i][r] * zs[1 + j][r]);
  }
  return out;
}

// Sine reverse for one row tile: adjoints of the h-streams in, of the z-streams out (in place)
template <int D>
__device__ __forceinline__ void sine_rev2(floatx4 (&hb)[HessGeo<D>::S], const floatx4 (&zs)[HessGeo<D>::S],
                                          const floatx4& sn, const floatx4& cs) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float wc = OMEGA * cs[r], ws = OMEGA2 * sn[r], w3c = OMEGA3 * cs[r];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) dot = fmaf(zs[1 + i][r], hb[1 + i][r], dot);
    float zb = wc * hb[0][r] - ws * dot;
    float tb[D];
#pragma unroll
    for (int i = 0; i < D; ++i) tb[i] = wc * hb[1 + i][r];
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j, ++p) {
        const float q = hb[1 + D + p][r], ti = zs[1 + i][r], tj = zs[1 + j][r];
        zb -= q * (ws * zs[1 + D + p][r] + w3c * (ti * tj));
        if (i == j) {
          tb[i] -= 2.f * ws * ti * q;
        } else {
          tb[i] -= ws * tj * q;
          tb[j] -= ws * ti * q;
        }
        hb[1 + D + p][r] = wc * q;
      }
#pragma unroll
    for (int i = 0; i < D; ++i) hb[1 + i][r] = tb[i];
    hb[0][r] = zb;
  }
}

// z-streams 1 .. S-1 of row tile rt at this lane's point: saved, or the first layer's rebuilt ones
// (l0 = l0_rebuilt(layer, L): tangents = the columns of W_0, second-order streams 0)
template <int NT, int D>
__device__ __forceinline__ void load_z2(const float* base, int rt, int lane, bool l0, const float* w0,
                                        floatx4 (&zs)[HessGeo<D>::S]) {
  constexpr int S = HessGeo<D>::S;
  zs[0] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (l0) {
    const float* p = w0 + (long)(16 * rt + 4 * (lane >> 4)) * D;
#pragma unroll
    for (int i = 0; i < D; ++i) zs[1 + i] = floatx4{p[i], p[D + i], p[2 * D + i], p[3 * D + i]};
#pragma unroll
    for (int s = 1 + D; s < S; ++s) zs[s] = floatx4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int s = 1; s < S; ++s) zs[s] = *reinterpret_cast<const floatx4*>(base + ((s * NT + rt) * 64 + lane) * 4);
  }
}

// sin / cos of w z of the saved value stream of row tile rt (one uniform fast / ocml choice per wave)
__device__ __forceinline__ void load_sc2(const float* base, int rt, int lane, floatx4& sn, floatx4& cs) {
  const floatx4 z = *reinterpret_cast<const floatx4*>(base + (rt * 64 + lane) * 4);
  float amax = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(OMEGA * z[r]));
  const bool big = wave_any_big(amax);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float sv, cv;
    if (big)
      sincosf(OMEGA * z[r], &sv, &cv);
    else
      sincos_fast(OMEGA * z[r], sv, cv);
    sn[r] = sv;
    cs[r] = cv;
  }
}

// ---------------------------------------------------------------------------
// forward: y (n, d_out), dy (n, d_out, D), hess (n, d_out, D, D) (both triangles), saved streams
// ---------------------------------------------------------------------------
template <int NT, int D>
__global__ __launch_bounds__(SplitGeo<NT>::THREADS) void jet_fwd_hess(
    const float* __restrict__ x, int N, int dout, int L, const float* __restrict__ prm, float* __restrict__ y,
    float* __restrict__ dy, float* __restrict__ hess, float* __restrict__ act) {
  using G = SplitGeo<NT>;
  static_assert(G::RPW == 1, "one row tile per wave (W <= 128)");
  constexpr int W = G::W, LDH = G::LDH, WV = G::WV, PLANE = G::PLANE, S = HessGeo<D>::S;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int ntiles = (int)act_tiles(N);
  const int tile = blockIdx.x;
  const int rt = wave;
  const int pt = tile * 16 + c;

  float xv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) xv[k] = pt < N ? x[(long)pt * D + k] : 0.f;

  floatx4 a[S];
  {  // layer 0 (K = d_in: VALU)
    const float* W0 = prm;
    const float* b0 = prm + (long)W * D;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * rt + 4 * g + r;
      float z = b0[n];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float w = W0[n * D + k];
        z = fmaf(w, xv[k], z);
        a[1 + k][r] = w;
      }
      a[0][r] = z;
#pragma unroll
      for (int s = 1 + D; s < S; ++s) a[s][r] = 0.f;
    }
  }
  for (int j = 0; j <= L; ++j) {
    if (j > 0) {
      // hidden layer j: B operands (layer j-1 activations) from LDS, A = W rows in registers
      const float* Wj = prm + hidden_off(D, W, j);
      const float* bj = Wj + (long)W * W;
      floatx4 wr[NT];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
        wr[kt] = *reinterpret_cast<const floatx4*>(Wj + ((16 * rt + c) * W + 16 * kt + 4 * g));
      a[0] = *reinterpret_cast<const floatx4*>(bj + 16 * rt + 4 * g);
#pragma unroll
      for (int s = 1; s < S; ++s) a[s] = floatx4{0.f, 0.f, 0.f, 0.f};
      // r outer: S independent accumulators between dependent MFMAs
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        floatx4 hv[S];
#pragma unroll
        for (int s = 0; s < S; ++s)
          hv[s] = *reinterpret_cast<const floatx4*>(lds + s * PLANE + c * LDH + 16 * kt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = 0; s < S; ++s) a[s] = mfma4(wr[kt][r], hv[s][r], a[s]);
      }
      __syncthreads();  // every wave has read layer j-1
    }
    if (act) {  // the first layer: its value stream only (l0_rebuilt, jet_common.hpp)
      const int ns = l0_rebuilt(j, L) ? 1 : S;
      float* base = act_base(act, j, ntiles, tile, S, NT);
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) *reinterpret_cast<floatx4*>(base + ((s * NT + rt) * 64 + lane) * 4) = a[s];
    }
    sine_jet2<D>(a);
    if (j < L) {
#pragma unroll
      for (int s = 0; s < S; ++s)
        *reinterpret_cast<floatx4*>(lds + s * PLANE + c * LDH + 16 * rt + 4 * g) = a[s];
      __syncthreads();
    }
  }
  // output layer: each wave sums its own neurons; the waves combine through LDS
  // (the activation planes are dead: every wave passed the last read barrier)
  float* red = lds;  // [WV][S][3][16]
  const float* Wo = prm + out_off(D, W, L);
  const float* bo = Wo + (long)dout * W;
  for (int o = 0; o < dout; ++o) {
    const floatx4 w4 = *reinterpret_cast<const floatx4*>(Wo + (o * W + 16 * rt + 4 * g));
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) v = fmaf(w4[r], a[s][r], v);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) red[((wave * S + s) * 3 + o) * 16 + c] = v;
    }
  }
  __syncthreads();
  if (wave == 0 && g == 0 && pt < N) {
    for (int o = 0; o < dout; ++o) {
      float tot[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        tot[s] = 0.f;
#pragma unroll
        for (int w = 0; w < WV; ++w) tot[s] += red[((w * S + s) * 3 + o) * 16 + c];
      }
      const long po = (long)pt * dout + o;
      y[po] = tot[0] + bo[o];
#pragma unroll
      for (int k = 0; k < D; ++k) dy[po * D + k] = tot[1 + k];
      int p = 0;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j, ++p) {
          hess[(po * D + i) * D + j] = tot[1 + D + p];
          hess[(po * D + j) * D + i] = tot[1 + D + p];
        }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: one partial-gradient row per block (the layout of insr_siren_jet_bwd's rows)
// ---------------------------------------------------------------------------
template <int NT, int D>
__global__ __launch_bounds__(SplitGeo<NT>::THREADS) void jet_bwd_hess(
    const float* __restrict__ x, int N, int dout, int L, const float* __restrict__ prm,
    const float* __restrict__ act, const float* __restrict__ gy, const float* __restrict__ gdy,
    const float* __restrict__ gh, float* __restrict__ part, long P) {
  using G = SplitGeo<NT>;
  static_assert(G::RPW == 1, "one row tile per wave (W <= 128)");
  constexpr int W = G::W, LDH = G::LDH, PLANE = G::PLANE, S = HessGeo<D>::S;
  constexpr int GS = hess_group<NT, D>(), NG = S / GS;
  static_assert(S % GS == 0, "the streams split into equal groups");
  constexpr int PLANEH = 16 * W;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* zbp = lds;               // zb of layer j, this group's streams   [sl][p][LDH]
  float* hpp = lds + GS * PLANE;  // h of layer j-1, this group's streams  [sl][m][16] (hT_index)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int ntiles = (int)act_tiles(N);
  const int tile = blockIdx.x;  // < ceil(N / 16): every tile a block reads was written by the forward
  const int rt = wave;
  const int pt = tile * 16 + c;
  const bool valid = pt < N;
  float* mypart = part + (long)blockIdx.x * P;

  float xv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) xv[k] = valid ? x[(long)pt * D + k] : 0.f;
  // adjoints of the output streams; the full (D, D) Hessian adjoint folds onto the pairs at load
  float ga[S][3];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int o = 0; o < 3; ++o) ga[s][o] = 0.f;
  if (valid) {
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      if (o >= dout) break;
      const long po = (long)pt * dout + o;
      if (gy) ga[0][o] = gy[po];
      if (gdy) {
#pragma unroll
        for (int k = 0; k < D; ++k) ga[1 + k][o] = gdy[po * D + k];
      }
      if (gh) {
        int p = 0;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int j = i; j < D; ++j, ++p)
            ga[1 + D + p][o] = (i == j) ? gh[(po * D + i) * D + i] : gh[(po * D + i) * D + j] + gh[(po * D + j) * D + i];
      }
    }
  }

  // ---- output layer ----
  floatx4 sn, cs, zs[S];
  {
    const float* baseL = act_base(act, L, ntiles, tile, S, NT);
    load_sc2(baseL, rt, lane, sn, cs);
    load_z2<NT, D>(baseL, rt, lane, l0_rebuilt(L, L), prm, zs);
  }
  const long wo_off = out_off(D, W, L);
  const float* Wo = prm + wo_off;
  floatx4 hb[S];
#pragma unroll
  for (int s = 0; s < S; ++s) hb[s] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    if (o >= dout) break;
    const floatx4 w4 = *reinterpret_cast<const floatx4*>(Wo + (o * W + 16 * rt + 4 * g));
    floatx4 acc4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const floatx4 hs = h_stream2<D>(s, zs, sn, cs);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc4[r] = fmaf(ga[s][o], hs[r], acc4[r]);
        hb[s][r] = fmaf(w4[r], ga[s][o], hb[s][r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = sum16(acc4[r]);
      if (c == 0) mypart[wo_off + (long)o * W + 16 * rt + 4 * g + r] = v;
    }
    if (wave == 0) {  // db_out[o]: every point counted once (lane group g == 0)
      const float v = sum16(g == 0 ? ga[0][o] : 0.f);
      if (lane == 0) mypart[wo_off + (long)dout * W + o] = v;
    }
  }

  // ---- sine layers j = L .. 0 ----
  for (int j = L; j >= 0; --j) {
    // the lane's coordinates again, opaque: no address derived from them is carried across the layer
    // loop in a register (the loop-carried state -- hb, zs, sin / cos -- is 84 registers at S = 10)
    int tq = threadIdx.x;
    asm volatile("" : "+v"(tq));
    const int lane = tq & 63, rt = tq >> 6, g = lane >> 4, c = lane & 15;
    // small widths: the propagation's W^T operand loaded at the top of the layer (its latency under the
    // sine reverse and the LDS exchange) and shared by the stream groups
    constexpr bool kHoistWT = NT <= 4;
    float wt[kHoistWT ? NT : 1][4];
    if constexpr (kHoistWT) {
      if (j > 0) {
        const float* Wj = prm + hidden_off(D, W, j);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) wt[kt][r] = Wj[(16 * kt + 4 * g + r) * W + 16 * rt + c];
      }
    }
    sine_rev2<D>(hb, zs, sn, cs);
    const long boff = (j == 0) ? (long)W * D : hidden_off(D, W, j) + (long)W * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = sum16(hb[0][r]);
      if (c == 0) mypart[boff + 16 * rt + 4 * g + r] = v;
    }
    if (j == 0) {
#pragma unroll
      for (int k = 0; k < D; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = sum16(fmaf(hb[0][r], xv[k], hb[1 + k][r]));
          if (c == 0) mypart[(long)(16 * rt + 4 * g + r) * D + k] = v;
        }
      break;
    }
    // sin / cos and z-streams of layer j-1: h_{j-1} now, the sine reverse of the next iteration
    floatx4 snp, csp, zp[S];
    {
      const float* basep = act_base(act, j - 1, ntiles, tile, S, NT);
      load_sc2(basep, rt, lane, snp, csp);
      load_z2<NT, D>(basep, rt, lane, l0_rebuilt(j - 1, L), prm, zp);
    }
    const float* Wj = prm + hidden_off(D, W, j);
    float* dW = mypart + hidden_off(D, W, j);
    floatx4 nh[S];
#pragma unroll
    for (int gr = 0; gr < NG; ++gr) {
      __syncthreads();  // the previous group's / layer's LDS readers are done
#pragma unroll
      for (int sl = 0; sl < GS; ++sl) {
        const int s = gr * GS + sl, col = 16 * rt + 4 * g;
        *reinterpret_cast<floatx4*>(zbp + sl * PLANE + c * LDH + col) = hb[s];
        const floatx4 hs = h_stream2<D>(s, zp, snp, csp);
        float* hp_s = hpp + sl * PLANEH;
#pragma unroll
        for (int r = 0; r < 4; ++r) hp_s[hT_index(col + r, c)] = hs[r];
      }
      __syncthreads();
      // dW_j, this wave's rows, this group's share: K = 16 points x GS streams (k = point 4g + r); a later
      // group adds to what this lane stored for the earlier ones (its own addresses of the block's row)
      constexpr int CTC = NT < 4 ? NT : 4;  // column tiles per accumulator pass (register budget)
#pragma unroll 1
      for (int ct0 = 0; ct0 < NT; ct0 += CTC) {
        floatx4 dacc[CTC];
#pragma unroll
        for (int ct = 0; ct < CTC; ++ct) dacc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < GS; ++sl) {
          const float* zb_s = zbp + sl * PLANE;
          const float* hp_s = hpp + sl * PLANEH;
          floatx4 a4, hv[CTC];
#pragma unroll
          for (int r = 0; r < 4; ++r) a4[r] = zb_s[(4 * g + r) * LDH + 16 * rt + c];
#pragma unroll
          for (int ct = 0; ct < CTC; ++ct)  // h(points 4g..4g+3, neuron 16 (ct0 + ct) + c)
            hv[ct] = *reinterpret_cast<const floatx4*>(hp_s + hT_index(16 * (ct0 + ct) + c, 4 * g));
          // r outer: CTC independent accumulators between dependent MFMAs
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ct = 0; ct < CTC; ++ct) dacc[ct] = mfma4(a4[r], hv[ct][r], dacc[ct]);
        }
#pragma unroll
        for (int ct = 0; ct < CTC; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* q = dW + (16 * rt + 4 * g + r) * W + 16 * (ct0 + ct) + c;
            *q = gr == 0 ? dacc[ct][r] : *q + dacc[ct][r];
          }
      }
      // propagate this group: hb_{j-1}[m] (this wave's rows) = sum_n W_j[n][m] zb[n]; A = W^T from L2
#pragma unroll
      for (int sl = 0; sl < GS; ++sl) nh[gr * GS + sl] = floatx4{0.f, 0.f, 0.f, 0.f};
      constexpr int KU = NT > 4 ? 2 : NT;  // bounded unroll: W^T loads in flight
#pragma unroll KU
      for (int kt = 0; kt < NT; ++kt) {
        float wa[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (kHoistWT)
            wa[r] = wt[kt][r];
          else
            wa[r] = Wj[(16 * kt + 4 * g + r) * W + 16 * rt + c];
        }
        floatx4 b4[GS];
#pragma unroll
        for (int sl = 0; sl < GS; ++sl)
          b4[sl] = *reinterpret_cast<const floatx4*>(zbp + sl * PLANE + c * LDH + 16 * kt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int sl = 0; sl < GS; ++sl) nh[gr * GS + sl] = mfma4(wa[r], b4[sl][r], nh[gr * GS + sl]);
      }
    }
    sn = snp;
    cs = csp;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      hb[s] = nh[s];
      zs[s] = zp[s];
    }
  }
}

// ---------------------------------------------------------------------------
// launchers: one 16-point tile per block
// ---------------------------------------------------------------------------
template <int NT, int D>
int launch_fwd_hess(const float* x, int N, int dout, int L, const float* prm, float* y, float* dy, float* hess,
                    float* act, hipStream_t st) {
  constexpr size_t lds = fwd_hess_lds_bytes<NT, D>();
  static_assert(lds <= kLdsMax, "the forward planes fit a CU's LDS");
  static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_fwd_hess<NT, D>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
  (void)attr_set;
  hipLaunchKernelGGL((jet_fwd_hess<NT, D>), dim3((N + 15) / 16), dim3(SplitGeo<NT>::THREADS), lds, st, x, N, dout, L,
                     prm, y, dy, hess, act);
  return (int)hipGetLastError();
}

template <int NT, int D>
int launch_bwd_hess(const float* x, int N, int dout, int L, const float* prm, const float* act, const float* gy,
                    const float* gdy, const float* gh, float* part, long P, hipStream_t st) {
  constexpr size_t lds = bwd_hess_lds_bytes<NT, D>();
  static_assert(lds <= kLdsMax, "a stream group's planes fit a CU's LDS");
  static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_bwd_hess<NT, D>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
  (void)attr_set;
  hipLaunchKernelGGL((jet_bwd_hess<NT, D>), dim3((N + 15) / 16), dim3(SplitGeo<NT>::THREADS), lds, st, x, N, dout, L,
                     prm, act, gy, gdy, gh, part, P);
  return (int)hipGetLastError();
}

}  // namespace insr
