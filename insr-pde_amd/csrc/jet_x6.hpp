// jet_x6.hpp -- tile-split SIREN jet kernels on the bf16 matrix cores with
// fp32-level accuracy ("bf16x6": every fp32 GEMM operand split in three bf16
// terms, six MFMA products per product pair).
//
// gfx950 has no xf32 path: the fp32 MFMA (v_mfma_f32_16x16x4_f32) runs at 1/16 of
// the bf16 rate.  An fp32 value a is split exactly enough into
//     a = a_h + a_m + a_l,   a_h = bf16(a), a_m = bf16(a - a_h), a_l = bf16(a - a_h - a_m)
// (8 + 8 + 8 significant bits, representation error <= 2^-26 |a|), and
//     a.b ~= a_m b_m + a_h b_l + a_l b_h + a_h b_m + a_m b_h + a_h b_h
// drops only terms <= 2^-26 |a||b| (a_m b_l, a_l b_m, a_l b_l).  Each bf16
// product is exact in fp32 and the MFMA accumulates in fp32, so a K-long dot
// product carries the error of an fp32 GEMM (K roundings of 2^-24) plus ~2^-25
// per term -- the same order as the reference's own fp32 addmm chain.  Six
// v_mfma_f32_16x16x32_bf16 (16 cycles each, K = 32) replace eight
// v_mfma_f32_16x16x4_f32 (32 cycles each) per 32-deep K chunk: 2.67x the matrix
// throughput of the exact-fp32 kernels in jet_split.hpp.
//
// Geometry and HBM layouts are those of jet_split.hpp (same saved-activation
// layout, same partial-gradient rows), so an x6 forward pairs with either
// backward.  What changes:
//   * the activations a block exchanges through LDS are stored pre-split, as
//     three bf16 planes [t][s][q = h,m,l][16 points][W + 8]; a B fragment
//     (8 consecutive neurons of one point) is one ds_read_b128 per plane;
//   * every wave splits its own weight rows (the A operand) at load.
// The K index of a 16x16x32 fragment is k = 8 (lane >> 4) + j, j = 0..7
// (A[row lane & 15][k], B[k][col lane & 15]); outputs keep the 16x16 C layout
// (rows 4 (lane >> 4) + r), which is what the sine jet and the saved layout use.
#pragma once
#include "jet_split.hpp"

namespace insr {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

// (a, b) -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32); a in the low half
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  const bf16x2v v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// three-term split of the pair (a, b): a = lo16(h) + lo16(m) + lo16(l), b likewise in the high halves
__device__ __forceinline__ void split3(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
  h = pk_bf16(a, b);
  float ra = a - bf_lo(h), rb = b - bf_hi(h);
  m = pk_bf16(ra, rb);
  ra -= bf_lo(m);
  rb -= bf_hi(m);
  l = pk_bf16(ra, rb);
}

// ---------------------------------------------------------------------------
// Precision template NQ = bf16 terms per operand (the planes of every LDS image):
//   NQ = 3  "x6"  a = a_h + a_m + a_l, six products (above): fp32-level accuracy
//   NQ = 2  "x3"  a = a_h + a_m (16 significant bits), products a_h b_m + a_m b_h + a_h b_h
//                 (dropped terms <= 2^-16 |a||b|): ~1e-5 relative per product
//   NQ = 1  "bf16" one product a_h b_h: bf16 operands, fp32 accumulation
//   NQ = 4  "f16x3" (forward only): a (scaled by a power of two) = a_h + a_l in FP16 terms
//                 (11 + 11 significant bits), products a_h b_l + a_l b_h + a_h b_h on
//                 v_mfma_f32_16x16x32_f16 (the bf16 rate), dropped a_l b_l <= 2^-22 |a||b|:
//                 fp32-level accuracy with half the x6 products.  fp16's range needs the
//                 scales: weights x 2^8 (kF16WScale, the planes), the Laplacian stream x 2^-4.
// The geometry, layouts and numerics contract are otherwise identical.
// ---------------------------------------------------------------------------
template <int NQ>
constexpr int np_of() { return NQ == 4 ? 2 : NQ; }  // LDS / fragment planes of a precision

template <int NQ>
struct FragQ {
  u32x4 q[np_of<NQ>()];  // q[0] = h, q[1] = m, q[2] = l
};

typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// (a, b) -> packed fp16 pair, round to nearest even; a in the low half
__device__ __forceinline__ unsigned pk_f16(float a, float b) {
  const f16x2v v = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, v);
}
using Frag3 = FragQ<3>;

// split of the pair (a, b) into NQ packed bf16 terms
template <int NQ>
__device__ __forceinline__ void splitq(float a, float b, unsigned (&o)[np_of<NQ>()]) {
  if constexpr (NQ == 4) {  // fp16 hi + lo (the caller applied the power-of-two scale)
    // the low terms a - float(hi) (exact) straight from the packed pair: one mixed-precision FMA each,
    // fma(hi, -1, a) with the fp16 half picked by op_sel -- 4 VALU ops per pair instead of the 8 of
    // convert / convert back / subtract per value (the compiler folds the C++ fma back into those)
    o[0] = pk_f16(a, b);
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(o[0]), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(o[0]), "v"(b));
    o[1] = pk_f16(ra, rb);
    return;
  }
  o[0] = pk_bf16(a, b);
  if constexpr (NQ > 1) {
    float ra = a - bf_lo(o[0]), rb = b - bf_hi(o[0]);
    o[1] = pk_bf16(ra, rb);
    if constexpr (NQ > 2) {
      ra -= bf_lo(o[1]);
      rb -= bf_hi(o[1]);
      o[2] = pk_bf16(ra, rb);
    }
  }
}

// 8 fp32 (k = j, j = 0..7: v0[0..3], v1[0..3]) -> one A/B fragment in NQ planes
template <int NQ>
__device__ __forceinline__ FragQ<NQ> split_frag(const floatx4& v0, const floatx4& v1) {
  unsigned t[4][np_of<NQ>()];
  splitq<NQ>(v0[0], v0[1], t[0]);
  splitq<NQ>(v0[2], v0[3], t[1]);
  splitq<NQ>(v1[0], v1[1], t[2]);
  splitq<NQ>(v1[2], v1[3], t[3]);
  FragQ<NQ> f;
#pragma unroll
  for (int q = 0; q < np_of<NQ>(); ++q) f.q[q] = u32x4{t[0][q], t[1][q], t[2][q], t[3][q]};
  return f;
}

__device__ __forceinline__ floatx4 mfma_bf(const u32x4& a, const u32x4& b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                 0, 0, 0);
}

__device__ __forceinline__ floatx4 mfma_h(const u32x4& a, const u32x4& b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// c += A B over one 32-deep K chunk (small terms first)
template <int NQ>
__device__ __forceinline__ floatx4 mfma_q(const FragQ<NQ>& a, const FragQ<NQ>& b, floatx4 c) {
  if constexpr (NQ == 4) {
    c = mfma_h(a.q[0], b.q[1], c);
    c = mfma_h(a.q[1], b.q[0], c);
    return mfma_h(a.q[0], b.q[0], c);
  }
  if constexpr (NQ == 3) {
    c = mfma_bf(a.q[1], b.q[1], c);
    c = mfma_bf(a.q[0], b.q[2], c);
    c = mfma_bf(a.q[2], b.q[0], c);
  }
  if constexpr (NQ >= 2) {
    c = mfma_bf(a.q[0], b.q[1], c);
    c = mfma_bf(a.q[1], b.q[0], c);
  }
  return mfma_bf(a.q[0], b.q[0], c);
}

// one fragment (8 consecutive bf16 of each plane) from NQ planes PLANE elements apart
template <int NQ, int PLANE>
__device__ __forceinline__ FragQ<NQ> lds_frag(const unsigned short* p) {
  FragQ<NQ> f;
#pragma unroll
  for (int q = 0; q < np_of<NQ>(); ++q) f.q[q] = *reinterpret_cast<const u32x4*>(p + q * PLANE);
  return f;
}

// 4 fp32 -> 4 consecutive bf16 of each of NQ planes (one b64 store per plane)
template <int NQ, int PLANE>
__device__ __forceinline__ void lds_put4(unsigned short* p, float a0, float a1, float a2, float a3) {
  unsigned u0[np_of<NQ>()], u1[np_of<NQ>()];
  splitq<NQ>(a0, a1, u0);
  splitq<NQ>(a2, a3, u1);
#pragma unroll
  for (int q = 0; q < np_of<NQ>(); ++q) *reinterpret_cast<u32x2*>(p + q * PLANE) = u32x2{u0[q], u1[q]};
}

template <int NT>
struct X6Geo {
  static constexpr int W = 16 * NT;
  static constexpr int WV = NT < 8 ? NT : 8;  // waves per block
  static constexpr int RPW = NT / WV;         // row tiles per wave
  static constexpr int KC = NT / 2;           // 32-deep K chunks of a hidden layer
  static constexpr int LDB = W + 8;           // point row of a bf16 plane (elements): conflict-free b128 reads
  static constexpr int PLANE = 16 * LDB;      // one (tile, stream, term) plane, bf16 elements
  static constexpr int THREADS = 64 * WV;
};

template <int NQ, int NT, int S, bool LAP, int T>
constexpr size_t fwd_x6_lds_bytes() {
  using G = X6Geo<NT>;
  // f16x3: + [2][T][waves] floats after the planes (the per-tile Laplacian-stream maxima, fwd_x6_block), the
  // tangent flags [2] and the rare branch's wave maxima [8]; a forward that leaves the bounds table
  // (act_has_bounds; LAP only matters at S = 3, 4): two classes of maxima, [2][T][2][waves]
  const size_t planes = (size_t)T * S * np_of<NQ>() * G::PLANE * 2 +
                        (act_has_bounds<NT, S, LAP>() ? (4 * T * 8 + 2 + 8) * sizeof(float)
                                                      : (NQ == 4 ? (2 * T * 8 + 2 + 8) * sizeof(float) : 0));
  const size_t red = (size_t)G::WV * T * S * 3 * 16 * sizeof(float);  // output-layer combine
  return planes > red ? planes : red;
}

// fragment (row tile rt, K chunk kc) of hidden layer j in orientation o (0: W_j rows, the
// forward's A operand; 1: W_j^T rows, the backward's) from the pre-split planes that follow
// the parameters (INSR_MODE_WSPLIT; capi.hip guarantees them): NQ of the 3 terms, one b128 each
__device__ __forceinline__ const u32x4* wsp_base(const float* prm, int din, int dout, int L, int W) {
  return reinterpret_cast<const u32x4*>(prm + wsplit_offset(din, dout, L, W));
}
template <int NQ, int NT>
__device__ __forceinline__ FragQ<NQ> wsp_frag(const u32x4* __restrict__ wsp, int L, int o, int j, int rt, int kc,
                                              int lane) {
  constexpr int W = 16 * NT, KC = NT / 2;
  if constexpr (NQ == 4) {  // the fp16 planes (o = 0: forward, o = 1: backward), after both bf16 orientations
    const u32x4* p = wsp + 2 * wsplit_orient_vecs(L, W) + o * wsplit_f16_vecs(L, W) +
                     ((((long)(j - 1) * NT + rt) * KC + kc) * 2) * 64 + lane;
    FragQ<NQ> f;
    f.q[0] = p[0];
    f.q[1] = p[64];
    return f;
  }
  const u32x4* p = wsp + o * wsplit_orient_vecs(L, W) + ((((long)(j - 1) * NT + rt) * KC + kc) * 3) * 64 + lane;
  FragQ<NQ> f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) f.q[q] = p[q * 64];
  return f;
}

// f16x3 (NQ = 4) operand scales of the forward: the value (sin, |h| <= 1) and tangent streams
// (|dh| <= w |t|) enter the fp16 products unscaled -- unless a layer's tangent bound leaves fp16's
// window (w |t| >= 2^15): then that layer's tangent planes take a block power of two too
// (fwd_x6_block, a uniform branch); the Laplacian stream
// (|ddh| <= w |q| + w^2 sum t^2: ~900x the tangents' square) is scaled per tile by the power of two
// 2^e that maps its bound's maximum into [2^14, 2^15) (fwd_x6_block); the products are unscaled by
// 2^-8 (the weights' scale) x 2^-e -- all exact
__device__ __forceinline__ int f16_exp_for(float m) {  // 2^e maps m into [2^14, 2^15); 0 for 0 / inf / NaN
  if (!(m > 0.f && m <= 3.0e38f)) return 0;
  int k;
  (void)frexpf(m, &k);
  return min(max(15 - k, -100), 100);
}
// The backward's h Laplacian stream (H planes, the dW B operand) takes the same bound, per block /
// dW slice: h_lap x 2^eh, z̄_lap x 2^-eh x the adjoints' 2^e (jet_bwd_x6, jet_bwd_x6p + dw_x6)

// Balanced tiles per block: with nbal > 0 the tiles of a batch are split over nbal blocks as
// evenly as possible (block b: tiles [b tiles / nbal, (b + 1) tiles / nbal), at most T), so a
// batch a little above a multiple of the resident block slots (16384 interior + 324 band
// points = 1045 tiles on 256 CUs) takes no extra block round; nbal = 0: T tiles per block.
__device__ __forceinline__ void block_tiles(int b, int N, int T, int nbal, int& tile0, int& cnt) {
  if (nbal > 0) {
    const long tiles = (N + 15) / 16;
    tile0 = (int)(((long)b * tiles) / nbal);
    cnt = (int)((((long)b + 1) * tiles) / nbal) - tile0;
  } else {  // T-tile blocks; the last one may hold fewer (T = 3 / 5 do not divide the act layout's 4)
    const int tiles = (N + 15) / 16;
    tile0 = b * T;
    cnt = tiles - tile0 < T ? tiles - tile0 : T;
  }
}

// The forward of one block (tiles tile0 .. tile0 + cnt - 1 of one network's batch): the body
// of jet_fwd_x6 and of jet_fwd_x6_multi (several networks / batches in one launch).
template <int NQ, int NT, int S, bool LAP, int T>
__device__ __forceinline__ void fwd_x6_block(const float* __restrict__ x, int N, int din, int dout, int L,
                                             const float* __restrict__ prm, float* __restrict__ y,
                                             float* __restrict__ dy, float* __restrict__ lap,
                                             float* __restrict__ act, const int tile0, const int cnt_rt) {
  using G = X6Geo<NT>;
  constexpr int W = G::W, RPW = G::RPW, LDB = G::LDB, WV = G::WV, PLANE = G::PLANE, KC = G::KC;
  constexpr int NTAN = LAP ? S - 2 : S - 1;
  // the tile count is a run-time value only for the balanced shapes (T = 3, 5): the T = 1, 2, 4
  // instantiations keep compile-time loops (a run-time guard there serialises the MFMA chains)
  const int cnt = (T == 3 || T == 5) ? cnt_rt : T;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  unsigned short* lds = reinterpret_cast<unsigned short*>(lds_f);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int ntiles = ((N + 63) / 64) * 4;
  const int rt0 = wave * RPW;
  const u32x4* wsp = wsp_base(prm, din, dout, L, W);
  // the waves' per-tile maxima of the tangent / Laplacian bounds of h_j (jet_common.hpp h_bounds)
  // [layer parity][T][class][8] after the planes: f16x3 Laplacian jets scale their Laplacian planes by the
  // tile's (LSC); a forward that saves the streams of a jet the saved-stream reverse sweep serves (TAB:
  // act_has_bounds) leaves both per tile in act for that sweep (act_bounds).  usl: the unscale of the next
  // layer's Laplacian-stream products per tile
  // (NC classes per tile: the Laplacian bound alone where no table is left -- those kernels are as they were)
  constexpr bool LSC = NQ == 4 && LAP, TAB = act_has_bounds<NT, S, LAP>();
  constexpr int NC = TAB ? 2 : 1, CL = NC - 1;  // CL: the Laplacian class
  float* zmx = lds_f + (T * S * np_of<NQ>() * PLANE) / 2;
  unsigned* zmxu = reinterpret_cast<unsigned*>(zmx);
  float usl[T];
#pragma unroll
  for (int t = 0; t < T; ++t) usl[t] = 1.f / kF16WScale;
  // f16x3 tangent streams: unscaled while every |dh| <= w |t| stays below 2^15 -- the common case,
  // fp16's window holds them with 22 bits.  A wave whose tangent bound leaves the window raises the
  // layer's LDS flag before the barrier the layer waits on anyway; every wave reads it after that
  // barrier, and only then (a uniform branch) the block exchanges its maxima and scales the layer's
  // tangent planes by the power of two 2^e that maps the block maximum into [2^14, 2^15) (layer 0:
  // t = the W_0 columns, bounded by every wave from W_0 itself).  ust: the next layer's tangent
  // unscale (block-uniform, scalar).
  float ust = 1.f / kF16WScale;
  int* tflag = reinterpret_cast<int*>(zmx + 2 * NC * T * 8);  // [2] by layer parity, then [8] wave maxima
  if constexpr (NQ == 4 && NTAN > 0) {
    if (threadIdx.x < 2) tflag[threadIdx.x] = 0;  // ordered before the first reader by layer 0's barrier
  }

  float xv[T][3];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int p = (tile0 + t) * 16 + c;
    for (int k = 0; k < 3; ++k) xv[t][k] = (t < cnt && p < N && k < din) ? x[(long)p * din + k] : 0.f;
  }

  floatx4 a[T][RPW][S];
  {  // layer 0 (K = d_in: VALU, exact fp32)
    const float* W0 = prm;
    const float* b0 = prm + (long)W * din;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * (rt0 + i) + 4 * g + r;
        const float bn = b0[n];
        float w0[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < din; ++k) w0[k] = W0[n * din + k];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          float z = bn;
          for (int k = 0; k < din; ++k) z = fmaf(w0[k], xv[t][k], z);
          a[t][i][0][r] = z;
#pragma unroll
          for (int k = 0; k < NTAN; ++k) a[t][i][1 + k][r] = w0[k];
          if constexpr (LAP) a[t][i][S - 1][r] = 0.f;
        }
      }
    }
  }
  for (int j = 0; j <= L; ++j) {
    if (j > 0) {
      const float* Wj = prm + hidden_off(din, W, j);
      const float* bj = Wj + (long)W * W;
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int rt = rt0 + i;
        FragQ<NQ> wf[KC];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) wf[kc] = wsp_frag<NQ, NT>(wsp, L, 0, j, rt, kc, lane);
        floatx4 bias = *reinterpret_cast<const floatx4*>(bj + 16 * rt + 4 * g);
        if constexpr (NQ == 4) bias *= kF16WScale;  // the fp16 products carry the weights' 2^8
#pragma unroll
        for (int t = 0; t < T; ++t) {
          a[t][i][0] = bias;
#pragma unroll
          for (int s = 1; s < S; ++s) a[t][i][s] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            if (t >= cnt) break;  // unused slots of a balanced block
#pragma unroll
            for (int s = 0; s < S; ++s) {
              const unsigned short* pb = lds + (t * S + s) * np_of<NQ>() * PLANE + c * LDB + 32 * kc + 8 * g;
              a[t][i][s] = mfma_q<NQ>(wf[kc], lds_frag<NQ, PLANE>(pb), a[t][i][s]);
            }
          }
        }
        if constexpr (NQ == 4) {  // undo the operand scales (powers of two: exact)
#pragma unroll
          for (int t = 0; t < T; ++t)
#pragma unroll
            for (int s = 0; s < S; ++s)
              a[t][i][s] *= (LAP && s == S - 1) ? usl[t] : (s > 0 ? ust : 1.f / kF16WScale);
        }
      }
    }
    // this wave's bounds of the h-streams of layer j per tile (before the barrier the next layer's operand
    // writes wait on anyway; j = 0 adds one for the f16x3 Laplacian jets -- the table's layer-0 pair of
    // the others comes from W_0, below): both classes in one packed reduction on the bit patterns
    if constexpr (TAB) {
      if (j < L && (LSC || (act && j > 0))) {
        int ln = lane;  // opaque: nothing derived from it is carried across the layer loop in a register
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int t = 0; t < T; ++t) {
          float mt, ml;
          h_bounds<S, LAP>(a[t][0], mt, ml);
          const unsigned w = bounds_wave_max(mt, ml, ln);
          if (ln < 2) zmxu[(((j & 1) * T + t) * 2 + ln) * 8 + wave] = w;
        }
      }
    } else if constexpr (LSC) {
      if (j < L) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
          float mt = 0.f;
#pragma unroll
          for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float t2 = 0.f;
#pragma unroll
              for (int k = 0; k < NTAN; ++k) t2 = fmaf(a[t][i][1 + k][r], a[t][i][1 + k][r], t2);
              mt = fmaxf(mt, fmaf(OMEGA, fabsf(a[t][i][S - 1][r]), OMEGA2 * t2));
            }
          mt = wave_max(mt);
          if (lane == 0) zmx[((j & 1) * T + t) * 8 + wave] = mt;
        }
      }
    }
    // f16x3 tangent streams of layer j's planes: this wave's bound w |t| against fp16's window
    auto tan_bound = [&]() -> float {
      float mt = 0.f;
      if (j == 0) {  // t = W_0 columns at every point: the bound of ALL rows, the same in every wave
        for (int n = lane; n < W; n += 64)
          for (int k = 0; k < NTAN; ++k) mt = fmaxf(mt, fabsf(prm[n * din + k]));
      } else {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int k = 0; k < NTAN; ++k)
#pragma unroll
              for (int r = 0; r < 4; ++r) mt = fmaxf(mt, fabsf(a[t][i][1 + k][r]));
      }
      return OMEGA * mt;
    };
    bool tbig = false;
    if constexpr (NQ == 4 && NTAN > 0) {
      if (j < L) {
        tbig = __any(tan_bound() >= 32768.f);
        if (j > 0 && tbig && lane == 0) tflag[j & 1] = 1;
      }
    }
    if (j > 0 || (NQ == 4 && LAP)) __syncthreads();  // every wave has read layer j-1 (and wrote its bounds)
    float sct = 1.f;  // this layer's tangent-plane scale
    if constexpr (NQ == 4 && NTAN > 0) {
      ust = 1.f / kF16WScale;
      if (j < L) {
        if (j > 0) tbig = __builtin_amdgcn_readfirstlane(tflag[j & 1]) != 0;
        if (tbig) {  // rare: the block maximum (layer 0: already every wave's own)
          float mt = wave_max(tan_bound());
          if (j > 0) {
            float* tmx = reinterpret_cast<float*>(tflag + 2);
            if (lane == 0) tmx[wave] = mt;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < WV; ++w) mt = fmaxf(mt, tmx[w]);
          }
          const int e = __builtin_amdgcn_readfirstlane(f16_exp_for(mt));
          sct = ldexpf(1.f, e);
          ust = ldexpf(1.f, -e) / kF16WScale;
        }
        if (j > 0 && threadIdx.x == 0) tflag[(j + 1) & 1] = 0;  // the other parity's readers passed the barrier
      }
    }
    if (act) {  // the first layer: its value stream only (l0_rebuilt, jet_common.hpp)
      const int ns = l0_rebuilt(j, L) ? 1 : S;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (t >= cnt) break;  // a balanced block's unused tile slots
        float* base = act_base(act, j, ntiles, tile0 + t, S, NT);
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int s = 0; s < S; ++s)
            if (s < ns) *reinterpret_cast<floatx4*>(base + ((s * NT + rt0 + i) * 64 + lane) * 4) = a[t][i][s];
      }
      if constexpr (TAB) {  // the bounds table: h_j's pair of every tile (jet_common.hpp act_bounds)
        if (j < L) {
          int tq = threadIdx.x;  // (opaque, as above)
          asm volatile("" : "+v"(tq));
          if (j > 0 || LSC) {  // the waves' slots, ordered by the barrier above: thread (t, class) folds them
            const int t = tq >> 1, cl = tq & 1;
            if (t < cnt && t < T) {
              const unsigned* q = zmxu + (((j & 1) * T + t) * 2 + cl) * 8;
              unsigned v = q[0];
#pragma unroll
              for (int w = 1; w < WV; ++w) v = max(v, q[w]);
              act_bounds(act, ntiles, tile0 + t, S, NT)[2 * j + cl] = __builtin_bit_cast(float, v);
            }
          } else if (tq < 64) {  // layer 0 without that barrier: W_0's pair, the same for every tile, by wave 0
            const unsigned w = l0_bounds_wave<S, LAP, W>(prm, din, tq);
            if (tq < 2) {
#pragma unroll
              for (int t = 0; t < T; ++t)
                if (t < cnt) act_bounds(act, ntiles, tile0 + t, S, NT)[tq] = __builtin_bit_cast(float, w);
            }
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) sine_jet<RPW, S, LAP>(a[t]);
    if (j < L) {
      float sll[T];  // this layer's Laplacian-stream operand scale per tile (f16x3)
#pragma unroll
      for (int t = 0; t < T; ++t) {
        sll[t] = 1.f;
        if constexpr (NQ == 4 && LAP) {
          const float* q = zmx + (((j & 1) * T + t) * NC + CL) * 8;
          float m = q[0];
#pragma unroll
          for (int w = 1; w < WV; ++w) m = fmaxf(m, q[w]);
          const int e = f16_exp_for(m);
          sll[t] = ldexpf(1.f, e);
          usl[t] = ldexpf(1.f, -e) / kF16WScale;
        }
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int s = 0; s < S; ++s) {
            unsigned short* pw = lds + (t * S + s) * np_of<NQ>() * PLANE + c * LDB + 16 * (rt0 + i) + 4 * g;
            const float sc = (LAP && s == S - 1) ? sll[t] : (s > 0 ? sct : 1.f);
            lds_put4<NQ, PLANE>(pw, sc * a[t][i][s][0], sc * a[t][i][s][1], sc * a[t][i][s][2], sc * a[t][i][s][3]);
          }
      __syncthreads();
    }
  }
  // output layer (exact fp32 VALU): each wave sums its own neurons, waves combine through LDS
  float* red = lds_f;  // [WV][T][S][3][16]
  const float* Wo = prm + out_off(din, W, L);
  const float* bo = Wo + (long)dout * W;
  for (int o = 0; o < dout; ++o) {
    float sv[T][S];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int s = 0; s < S; ++s) sv[t][s] = 0.f;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const floatx4 w4 = *reinterpret_cast<const floatx4*>(Wo + (o * W + 16 * (rt0 + i) + 4 * g));
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = 0; s < S; ++s) sv[t][s] = fmaf(w4[r], a[t][i][s][r], sv[t][s]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        float v = sv[t][s];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) red[(((wave * T + t) * S + s) * 3 + o) * 16 + c] = v;
      }
  }
  __syncthreads();
  static_assert(T <= 4 * WV, "output stage: one lane group per tile");
  if (wave * 4 + g < cnt) {  // lane group g of wave w finishes tile 4 w + g
    const int t = wave * 4 + g;
    const int p = (tile0 + t) * 16 + c;
    if (p < N) {
      for (int o = 0; o < dout; ++o) {
        float tot[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          tot[s] = 0.f;
#pragma unroll
          for (int w = 0; w < WV; ++w) tot[s] += red[(((w * T + t) * S + s) * 3 + o) * 16 + c];
        }
        y[(long)p * dout + o] = tot[0] + bo[o];
        if (dy)
          for (int k = 0; k < NTAN; ++k) dy[((long)p * dout + o) * din + k] = tot[1 + k];
        if constexpr (LAP) {
          if (lap) lap[(long)p * dout + o] = tot[S - 1];
        }
      }
    }
  }
}

// register cap of the single-network forward: 4 waves / SIMD (two 512-thread blocks per CU)
// where the body fits 128 VGPRs without spilling (unconstrained, T = 2 takes ~200).  W = 256
// 4-stream gradient jets (elasticity3Dbunny's 3-d gradient): 125 VGPRs in round 3, 131 after the
// f16x3 tangent-stream guard -- one block per CU instead of two, the forward 2.39 -> 3.59 ms per step
template <int NQ, int NT, int S, bool LAP, int T>
constexpr int x6_fwd_min_waves() {  // (the bf16x6 variant of the W = 256 case would spill 14 VGPRs)
  return ((NT == 8 && (S == 1 || (S == 3 && T <= 2))) || (NQ == 4 && NT == 16 && S == 4 && !LAP && T == 1))
             ? 4
             : 1;  // capped vs uncapped: kbench r2s21
}

template <int NQ, int NT, int S, bool LAP, int T>
__global__ __launch_bounds__(X6Geo<NT>::THREADS, (x6_fwd_min_waves<NQ, NT, S, LAP, T>())) void jet_fwd_x6(
    const float* __restrict__ x, int N, int din, int dout, int L, const float* __restrict__ prm,
    float* __restrict__ y, float* __restrict__ dy, float* __restrict__ lap, float* __restrict__ act, int nbal) {
  int tile0, cnt;
  block_tiles(blockIdx.x, N, T, nbal, tile0, cnt);
  fwd_x6_block<NQ, NT, S, LAP, T>(x, N, din, dout, L, prm, y, dy, lap, act, tile0, cnt);
}

// Horizontal fusion: up to kFwdJobs independent forward jets of one architecture and jet
// mode (different networks and/or batches, e.g. the frozen previous velocity field and the
// trainable one at the same collocation points, plus the boundary band) in ONE launch.  A
// value jet of 16384 points fills one 8-wave block per CU and is latency-bound (layer-serial
// chain); two such jets side by side keep two blocks per CU in flight, so one launch costs
// well under two.  Small jobs (a boundary band of a few hundred points) run 1-tile blocks
// (TB) placed FIRST in the grid: they take a slot on a few CUs, finish in about half the
// time of a TA-tile block, and the remaining TA blocks take their slots -- instead of a
// latency-bound launch of their own.  Blocks [first[k], first[k + 1]) belong to job k; the
// per-point arithmetic is that of jet_fwd_x6 (same results bit for bit, any T).
struct FwdJobsX6 {
  InsrJetJob job[kFwdJobs];
  int first[kFwdJobs + 1];
  int small[kFwdJobs];  // 1: the job runs TB-tile blocks
  int nbal[kFwdJobs];   // > 0: the job's tiles balanced over its nbal TA-tile blocks
  int njobs;
};

// value and 2-d gradient jets at W = 128: hold the kernel to 128 VGPRs (4 waves per SIMD = two
// 8-wave blocks per CU), which the value TA = 4 body meets on its own (116), the gradient
// TA = 2 and the 1-tile bodies are scheduled into without spills
template <int NQ, int NT, int S, bool LAP, int TA>
constexpr int x6_multi_min_waves() {  // + the W = 256 4-stream gradient case of x6_fwd_min_waves
  return ((NT == 8 && (S == 1 || S == 3)) || (NQ == 4 && NT == 16 && S == 4 && !LAP && TA == 1)) ? 4 : 1;
}

template <int NQ, int NT, int S, bool LAP, int TA, int TB>
__global__ __launch_bounds__(X6Geo<NT>::THREADS, (x6_multi_min_waves<NQ, NT, S, LAP, TA>())) void jet_fwd_x6_multi(
    const FwdJobsX6 jobs, int din, int dout, int L) {
  const int b = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int q = 1; q < kFwdJobs; ++q) k += (q < jobs.njobs && b >= jobs.first[q]) ? 1 : 0;
  const InsrJetJob& jb = jobs.job[k];
  const int dout_k = jb.d_out > 0 ? jb.d_out : dout;
  if constexpr (TA != TB) {
    if (jobs.small[k]) {
      fwd_x6_block<NQ, NT, S, LAP, TB>(jb.x, (int)jb.n, din, dout_k, L, jb.params, jb.y, jb.dy, jb.lap, jb.act,
                                       (b - jobs.first[k]) * TB, TB);
      return;
    }
  }
  int tile0, cnt;
  block_tiles(b - jobs.first[k], (int)jb.n, TA, jobs.nbal[k], tile0, cnt);
  fwd_x6_block<NQ, NT, S, LAP, TA>(jb.x, (int)jb.n, din, dout_k, L, jb.params, jb.y, jb.dy, jb.lap, jb.act, tile0, cnt);
}

// Mixed-mode horizontal fusion: independent forward jets of one width and d_in but DIFFERENT
// jet modes (the pressure phase's detached velocity Jacobian beside the pressure Laplacian
// jet; the projection's two value jets beside the pressure gradient) in ONE launch.  Each
// block runs one job with that job's own body and tile count (value T = 2, gradient and
// Laplacian T = 1: the forward tile policy at W = 128), so outputs are bit-identical to the
// job's own launch; the kernel's registers / LDS are the largest body's.
struct FwdMixX6 {
  InsrJetJob job[kFwdJobs];
  int first[kFwdJobs + 1];
  int mode[kFwdJobs];     // INSR_MODE_VALUE / GRAD / LAP / INSR_MIX_ADVECT
  float sc[kFwdJobs][3];  // INSR_MIX_ADVECT: dt, lo, hi
  int njobs;
};

// BODIES: the job kinds a kernel instance carries (bit m = jet mode m, bit 3 = INSR_MIX_ADVECT):
// its registers and LDS are those of the largest body it holds, so a launch takes the smallest
// instance that covers its jobs (value + advect: 62 VGPRs, four blocks per CU; with a
// Laplacian body: 90)
constexpr int kMixV = 1, kMixG = 2, kMixL = 4, kMixA = 8;
// tiles per block of the advection target job (its two value jets run back to back in one block: the
// longest chain of the advection phase's launch)
#ifndef INSR_MIX_ADV_T
#define INSR_MIX_ADV_T 2
#endif
constexpr int kMixAdvT = INSR_MIX_ADV_T;

template <int NQ, int NT, int DIN, int BODIES>
constexpr size_t fwd_mix_lds_bytes() {
  constexpr size_t a = (BODIES & (kMixV | kMixA)) ? fwd_x6_lds_bytes<NQ, NT, 1, false, 2>() : 0;
  constexpr size_t b = (BODIES & kMixG) ? fwd_x6_lds_bytes<NQ, NT, 1 + DIN, false, 1>() : 0;
  constexpr size_t c = (DIN <= 2 && (BODIES & kMixL)) ? fwd_x6_lds_bytes<NQ, NT, 2 + DIN, true, 1>() : 0;
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// with a Laplacian body: 6 waves per SIMD (80 VGPRs, 11 spills; three blocks per CU) measured
// 0.5% faster per headline step than 4 (profiles/r02/mix_lap_waves_ab)
template <int NQ, int NT, int DIN, int BODIES>
__global__ __launch_bounds__(X6Geo<NT>::THREADS, (BODIES & kMixL) ? 6 : 4) void jet_fwd_x6_mixed(const FwdMixX6 jobs,
                                                                                              int dout, int L) {
  const int b = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int q = 1; q < kFwdJobs; ++q) k += (q < jobs.njobs && b >= jobs.first[q]) ? 1 : 0;
  const InsrJetJob& jb = jobs.job[k];
  const int dk = jb.d_out > 0 ? jb.d_out : dout;
  const int lb = b - jobs.first[k];
  int tile0, cnt;
  switch (jobs.mode[k]) {
    case INSR_MODE_VALUE:
      if constexpr ((BODIES & kMixV) != 0) {
        block_tiles(lb, (int)jb.n, 2, 0, tile0, cnt);
        fwd_x6_block<NQ, NT, 1, false, 2>(jb.x, (int)jb.n, DIN, dk, L, jb.params, jb.y, jb.dy, jb.lap, jb.act, tile0,
                                          cnt);
      }
      break;
    case INSR_MODE_GRAD:
      if constexpr ((BODIES & kMixG) != 0)
        fwd_x6_block<NQ, NT, 1 + DIN, false, 1>(jb.x, (int)jb.n, DIN, dk, L, jb.params, jb.y, jb.dy, jb.lap, jb.act,
                                                lb, 1);
      break;
    case INSR_MODE_LAP:
      if constexpr (DIN <= 2 && (BODIES & kMixL) != 0)
        fwd_x6_block<NQ, NT, 2 + DIN, true, 1>(jb.x, (int)jb.n, DIN, dk, L, jb.params, jb.y, jb.dy, jb.lap, jb.act,
                                               lb, 1);
      break;
    case INSR_MIX_ADVECT: {  // y = f(clamp(x - dt f(x), lo, hi)), f(x) -> dy, the foot -> lap
      if constexpr ((BODIES & kMixA) == 0) break;
      // (fluid/model.py:96-97; every quantity of a point stays in its block: one launch for
      // the frozen field's two value jets and the foot between them)
      const int n = (int)jb.n;
      block_tiles(lb, n, kMixAdvT, 0, tile0, cnt);
      float* up = jb.dy;
      float* foot = jb.lap;
      fwd_x6_block<NQ, NT, 1, false, kMixAdvT>(jb.x, n, DIN, dk, L, jb.params, up, nullptr, nullptr, nullptr, tile0,
                                               cnt);
      // the block's own global writes, read back by its other waves: workgroup scope (the
      // stores drain before the barrier; the lines were never cached in this CU's L1)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __syncthreads();
      const float a = -jobs.sc[k][0], lo = jobs.sc[k][1], hi = jobs.sc[k][2];
      for (int i = threadIdx.x; i < cnt * 16 * DIN; i += blockDim.x) {
        const long p = (long)tile0 * 16 + i / DIN;
        const int kk = i % DIN;
        if (p < n) foot[p * DIN + kk] = fminf(fmaxf(fmaf(a, up[p * dk + kk], jb.x[p * DIN + kk]), lo), hi);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __syncthreads();
      fwd_x6_block<NQ, NT, 1, false, kMixAdvT>(foot, n, DIN, dk, L, jb.params, jb.y, nullptr, nullptr, nullptr, tile0,
                                               cnt);
      break;
    }
    default:  // never reached: the host validates every job's mode (mixed_jobs_ok, capi.hip)
      break;
  }
}

template <int NQ, int NT, int DIN, int BODIES>
int launch_fwd_x6_mixed_t(const InsrJetJob* jobs, const int* modes, const float* scalars, int njobs, int dout, int L,
                          hipStream_t st) {
  constexpr size_t lds = fwd_mix_lds_bytes<NQ, NT, DIN, BODIES>();
  if constexpr (lds > kLdsMax) {
    return INSR_EINVAL;
  } else {
    if (njobs < 1 || njobs > kFwdJobs) return INSR_EINVAL;
    static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_fwd_x6_mixed<NQ, NT, DIN, BODIES>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
    (void)attr_set;
    FwdMixX6 pk{};
    int nb = 0;
    for (int k = 0; k < njobs; ++k) {
      if (modes[k] == INSR_MODE_LAP && DIN > 2) return INSR_EINVAL;
      pk.job[k] = jobs[k];
      pk.mode[k] = modes[k];
      for (int q = 0; q < 3; ++q) pk.sc[k][q] = scalars ? scalars[3 * k + q] : 0.f;
      pk.first[k] = nb;
      const long tiles = (jobs[k].n + 15) / 16;
      nb += (int)(modes[k] == INSR_MODE_VALUE ? (tiles + 1) / 2
                                              : (modes[k] == INSR_MIX_ADVECT ? (tiles + kMixAdvT - 1) / kMixAdvT : tiles));
    }
    pk.first[njobs] = nb;
    pk.njobs = njobs;
    if (nb == 0) return 0;
    hipLaunchKernelGGL((jet_fwd_x6_mixed<NQ, NT, DIN, BODIES>), dim3(nb), dim3(X6Geo<NT>::THREADS), lds, st, pk, dout,
                       L);
    return (int)hipGetLastError();
  }
}

// small[k] != 0: job k runs 1-tile blocks (ignored when T == 1)
template <int NQ, int NT, int S, bool LAP, int T>
int launch_fwd_x6_multi_t(const InsrJetJob* jobs, const int* small, const int* nbal, int njobs, int din, int dout,
                          int L, hipStream_t st) {
  // 1-tile blocks for small jobs only beside T >= 4 blocks: with T <= 2 the second body would
  // raise the kernel's registers (T = 2 value: 84 vs 62 VGPRs, two blocks per CU fewer)
  constexpr int TB = T <= 2 ? T : 1;
  constexpr size_t lds = fwd_x6_lds_bytes<NQ, NT, S, LAP, T>();
  if constexpr (lds > kLdsMax) {
    return INSR_EINVAL;
  } else {
    if (njobs < 1 || njobs > kFwdJobs) return INSR_EINVAL;
    static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_fwd_x6_multi<NQ, NT, S, LAP, T, TB>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
    (void)attr_set;
    FwdJobsX6 pk{};
    int nb = 0, m = 0;
    for (int pass = 0; pass < 2; ++pass)  // small jobs' blocks first
      for (int k = 0; k < njobs; ++k) {
        const int sm = (T != TB && small && small[k]) ? 1 : 0;
        if (sm != 1 - pass) continue;
        pk.job[m] = jobs[k];
        pk.small[m] = sm;
        pk.nbal[m] = sm ? 0 : (nbal ? nbal[k] : 0);
        pk.first[m] = nb;
        const int t = sm ? TB : T;
        nb += pk.nbal[m] > 0 ? pk.nbal[m] : (int)(((jobs[k].n + 15) / 16 + t - 1) / t);
        ++m;
      }
    pk.first[njobs] = nb;
    pk.njobs = njobs;
    if (nb == 0) return 0;
    hipLaunchKernelGGL((jet_fwd_x6_multi<NQ, NT, S, LAP, T, TB>), dim3(nb), dim3(X6Geo<NT>::THREADS), lds, st, pk, din,
                       dout, L);
    return (int)hipGetLastError();
  }
}

template <int NQ, int NT, int S, bool LAP, int T>
int launch_fwd_x6_t(const float* x, int N, int din, int dout, int L, const float* prm, float* y, float* dy,
                    float* lap, float* act, int nbal, hipStream_t st) {
  constexpr size_t lds = fwd_x6_lds_bytes<NQ, NT, S, LAP, T>();
  if constexpr (lds > kLdsMax) {
    return INSR_EINVAL;
  } else {
    const int nb = ((N + 15) / 16 + T - 1) / T;
    static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_fwd_x6<NQ, NT, S, LAP, T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds), true);  // once per instantiation (thread-safe static init)
    (void)attr_set;
    if (N < 0) {  // occupancy query (split_tiles): resident blocks per CU
      int occ = 0;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)jet_fwd_x6<NQ, NT, S, LAP, T>, X6Geo<NT>::THREADS, lds);
      return occ;
    }
    hipLaunchKernelGGL((jet_fwd_x6<NQ, NT, S, LAP, T>), dim3(nbal > 0 ? nbal : nb), dim3(X6Geo<NT>::THREADS), lds, st,
                       x, N, din, dout, L, prm, y, dy, lap, act, nbal);
    return (int)hipGetLastError();
  }
}

}  // namespace insr

namespace insr {

// ---------------------------------------------------------------------------
// backward.  Per layer j (after the lane-local sine reverse, zb in registers):
//   for each stream group (SG streams of all T tiles -- the LDS holds one group):
//     write zb  -> Z planes, point-major  [set][q][16 p][W + 8]   (b64 per plane)
//           h_{j-1} (rebuilt from the saved z + sin/cos)
//              -> H planes, neuron-major [set][q][W][16 p]        (b16 per plane)
//     dW_j (this wave's rows n, all columns m):  K = (set, point) in 32-deep chunks of
//           two 16-point sets; A = zb[n][p] (column reads of Z), B = h[m][p] (one b128
//           per plane of H); accumulates over the groups in registers
//     propagation of the group's streams:  hb_{j-1}[m] = sum_n W[n][m] zb[n];
//           A = W^T rows m of this wave (strided L2 loads, split once per layer),
//           B = Z rows (one b128 per plane)
// ---------------------------------------------------------------------------
// LDS images are pre-split bf16 planes (the producer splits each value once):
// Z [set][q][16 p][W + 8], H [set][q][W][16 p]; the dW A operand comes from u16 column
// reads of Z.  (Measured alternative, fp32 planes split by every reader: 1.4-2x slower --
// the reader-side split is 8x redundant VALU work across the block's waves.)
// h-stream s of a sine layer from the derivative z-streams held in registers
// (zd[s - 1] = stream s >= 1; never read at S = 1) + sin/cos
template <int S, bool LAP>
__device__ __forceinline__ floatx4 h_from_regs(int s, const floatx4* zd, const floatx4& sn, const floatx4& cs) {
  constexpr int NTAN = LAP ? S - 2 : S - 1;
  if (s == 0) return sn;
  floatx4 out;
  if (LAP && s == S - 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float t2 = 0.f;
#pragma unroll
      for (int i = 0; i < NTAN; ++i) t2 = fmaf(zd[i][r], zd[i][r], t2);
      out[r] = OMEGA * cs[r] * zd[s - 1][r] - OMEGA2 * sn[r] * t2;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = OMEGA * cs[r] * zd[s - 1][r];
  }
  return out;
}

// Scheduling fence between the unrolled fragment iterations of the backward: keeps the
// compiler from hoisting every iteration's LDS reads to the top (register spills);
// the MFMAs of one iteration still cover the next iteration's reads of the other wave.
#define X6_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// 4x4 transpose across a lane quad (lanes c & ~3 .. c | 3 of one lane group g): in, lane c
// holds v[r] = M[neuron 4g + r][point c]; out, lane c holds neuron 4g + (c & 3) at points
// (c & ~3) + r.  Two DPP exchange stages (lane ^ 1, lane ^ 2); every lane must be active.
__device__ __forceinline__ float dpp_xor1(float v) {  // quad_perm 1,0,3,2
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_xor2(float v) {  // quad_perm 2,3,0,1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
}
__device__ __forceinline__ floatx4 quad_transpose(const floatx4& v, int c) {
  const bool o1 = c & 1, o2 = c & 2;
  const float s0 = dpp_xor1(o1 ? v[0] : v[1]), s1 = dpp_xor1(o1 ? v[2] : v[3]);
  const floatx4 a = {o1 ? s0 : v[0], o1 ? v[1] : s0, o1 ? s1 : v[2], o1 ? v[3] : s1};
  const float t0 = dpp_xor2(o2 ? a[0] : a[2]), t1 = dpp_xor2(o2 ? a[1] : a[3]);
  return floatx4{o2 ? t0 : a[0], o2 ? t1 : a[1], o2 ? a[2] : t0, o2 ? a[3] : t1};
}

// ds_read_b64_tr_b16 (gfx950 LDS transpose read, 8-B aligned address in LDS)
typedef short v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s ds_read_tr16(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
}

// one fragment by column reads of a point-major image (NQ planes PLANE elements apart, point rows
// ROW elements apart) with the transpose read: per 16-lane group, lane 4 r + p4 addresses point row
// r (+ 4), columns 4 p4 .. 4 p4 + 3 of 16 neurons -- p is that address in plane 0 -- and lane c
// receives neuron c at the 8 points (2 reads per plane instead of 8 u16 reads; every lane takes
// part: EXEC full).  Zeros when !live.  The statement order is load-bearing:
// the select stays inside, on the assembled vector, and a caller that keeps the fragment copies it plane
// by plane (a whole-struct copy or initialisation reorders the reads in some instantiations)
template <int NQ, int PLANE, int ROW>
__device__ __forceinline__ FragQ<NQ> lds_frag_tr(const unsigned short* p, bool live = true) {
  FragQ<NQ> f;
#pragma unroll
  for (int q = 0; q < np_of<NQ>(); ++q) {
    const v4s lo = ds_read_tr16(p + q * PLANE);
    const v4s hi = ds_read_tr16(p + q * PLANE + 4 * ROW);
    const u32x2 wl = __builtin_bit_cast(u32x2, lo), wh = __builtin_bit_cast(u32x2, hi);
    f.q[q] = live ? u32x4{wl[0], wl[1], wh[0], wh[1]} : u32x4{0u, 0u, 0u, 0u};
  }
  return f;
}

// one value granule (4 neurons x 1 point per lane, C layout) -> neuron-major bf16 planes
// [q][m][16 p] at row0 = first neuron of the lane group: quad transpose, then one b64
// store of 4 consecutive points per plane (instead of 12 b16 stores)
template <int NQ, int PLANE>
__device__ __forceinline__ void put_neuron_major(unsigned short* P, const floatx4& v, int row0, int c) {
  const floatx4 tv = quad_transpose(v, c);
  lds_put4<NQ, PLANE>(P + (row0 + (c & 3)) * 16 + (c & ~3), tv[0], tv[1], tv[2], tv[3]);
}

// LDS images of one stream group: Z point-major [q][16 p][W + 8] (the propagation B operand,
// and the dW A operand through u16 column reads), H neuron-major [q][m][16 p] (the dW B
// operand, one b128 per plane; written through a quad transpose: one b64 store per plane;
// x6_bwd_pm shapes: H as Z, ZSET elements per set).
template <int NQ, int NT>
struct X6BwdGeo {
  using G = X6Geo<NT>;
  static constexpr int W = G::W;
  static constexpr int ZROW = G::LDB;                  // elements of a Z point row
  static constexpr int ZPLANE = 16 * ZROW;
  static constexpr int ZSET = np_of<NQ>() * ZPLANE + 32;  // +16 dwords: the four lane groups of a
                                                          // column read hit disjoint banks
  static constexpr int HPLANE = W * 16;
  static constexpr int HSET = np_of<NQ>() * HPLANE;
  static constexpr size_t SET_BYTES = (size_t)(ZSET + HSET) * 2;
};

// The f16x3 value backward at W = 128 (one row tile per wave, one stream group) keeps H point-major
// like Z -- [q][16 p][W + 8], one lds_put4 per granule, no quad transpose -- and reads both dW
// operands with the transpose read; its waves tile dW 2 row tiles x 4 column tiles (jet_bwd_x6)
template <int NQ, int NT, int S>
constexpr bool x6_bwd_pm() {
  return NQ == 4 && NT == 8 && S == 1;
}
template <int NQ, int NT, int S>
constexpr size_t x6_bwd_set_bytes() {
  using BG = X6BwdGeo<NQ, NT>;
  return x6_bwd_pm<NQ, NT, S>() ? (size_t)2 * BG::ZSET * 2 : BG::SET_BYTES;
}

// streams per LDS group: all S if T tiles of them fit, else S/2, else 1
template <int NQ, int NT, int S, int T>
constexpr int x6_bwd_sg() {
  constexpr size_t set = x6_bwd_set_bytes<NQ, NT, S>();
  if ((size_t)T * S * set <= kLdsMax) return S;
  if (S % 2 == 0 && (size_t)T * (S / 2) * set <= kLdsMax) return S / 2;
  return 1;
}

// value jets (S = 1) take in-kernel adjoint seeds (BwdJobsX6::seeds): the block's seeds [T][3][16] and
// the waves' square sums [8][INSR_SEED_MAX] after the maxima
template <int S, int T>
constexpr size_t bwd_x6_seed_floats() {
  return S == 1 ? (size_t)T * 48 + 8 * INSR_SEED_MAX : 0;
}
template <int NQ, int NT, int S, int T>
constexpr size_t bwd_x6_lds_bytes() {  // + 2 x 5 x 8 floats: the waves' per-layer maxima (NQ = 4)
  return (size_t)T * x6_bwd_sg<NQ, NT, S, T>() * x6_bwd_set_bytes<NQ, NT, S>() + 2 * 5 * 8 * sizeof(float) +
         bwd_x6_seed_floats<S, T>() * sizeof(float);
}

template <int NQ, int NT, int S, bool LAP, int T>
__global__ __launch_bounds__(X6Geo<NT>::THREADS) void jet_bwd_x6(const BwdJobsX6 J, int din, int dout, int L,
                                                                  const float* __restrict__ prm,
                                                                  float* __restrict__ part, long P) {
  using G = X6Geo<NT>;
  using BG = X6BwdGeo<NQ, NT>;
  constexpr int W = G::W, RPW = G::RPW, KC = G::KC;
  constexpr bool PM = x6_bwd_pm<NQ, NT, S>();  // point-major H, tiled dW, streamed W^T
  constexpr int LDB = BG::ZROW, ZPLANE = BG::ZPLANE, ZSET = BG::ZSET, HPLANE = BG::HPLANE;
  constexpr int HSET = PM ? BG::ZSET : BG::HSET;
  constexpr int NTAN = LAP ? S - 2 : S - 1;
  constexpr int SG = x6_bwd_sg<NQ, NT, S, T>();
  constexpr int NG = S / SG;            // stream groups per layer
  constexpr int NSET = T * SG;          // 16-point sets per group
  constexpr int NCH = (NSET + 1) / 2;   // 32-deep K chunks of the weight gradient
  static_assert(S % SG == 0, "stream groups");
  static_assert(NG == 1 || RPW * NT <= 16, "dW accumulators across groups");
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  unsigned short* Z = reinterpret_cast<unsigned short*>(lds_f);
  unsigned short* H = Z + NSET * ZSET;
  // NQ = 4, [2][5][waves]: each wave's per-layer max |z̄| over the value stream, the Laplacian stream, its
  // bound of h_{j-1}'s Laplacian stream, max |z̄| over the tangent streams, its bound of h_{j-1}'s tangents
  float* zred = lds_f + NSET * (ZSET + HSET) / 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  // NQ = 4 (INSR_BWD_F16_FUSED, the x6 backward's products on the fp16 matrix cores): per layer the
  // block's z̄ is scaled by the power of two 2^e that maps its largest |z̄| (Laplacian stream x 16)
  // into [2^14, 2^15), h's Laplacian stream by 2^-4 and W^T comes from the fp16 backward planes
  // (x 2^8); dW is unscaled by 2^-e, the propagation by 2^-(8 + e) -- exact powers of two
  // this block's job (a batch of the launch's network) and its tiles within that batch
  const int b = blockIdx.x;
  int jk = 0;
#pragma unroll
  for (int q = 1; q < kBwdJobs; ++q) jk += (q < J.njobs && b >= J.first[q]) ? 1 : 0;
  const float* __restrict__ x = J.x[jk];
  const float* __restrict__ act = J.act[jk];
  const float* __restrict__ gy = J.gy[jk];
  const float* __restrict__ gdy = J.gdy[jk];
  const float* __restrict__ glap = J.glap[jk];
  const int N = J.n[jk];
  const int ntiles = ((N + 63) / 64) * 4;
  int tile0, cnt_rt;
  block_tiles(b - J.first[jk], N, T, J.nbal[jk], tile0, cnt_rt);
  const int cnt = (T == 3 || T == 5) ? cnt_rt : T;  // run-time only for the balanced shapes
  // tile of slot t for memory reads: a slot past the batch's last tile (a balanced block's unused
  // slot, or the tail of a T-tile block) re-reads the block's first tile -- saved streams the
  // forward wrote (its own T may have been smaller: tiles past ceil(n / 16) hold no data) -- and
  // its adjoints and x are zero, so it contributes nothing
  auto tt = [&](int t) { return tile0 + (t < cnt_rt ? t : 0); };
  const int rt0 = wave * RPW;
  float* mypart = part + (long)blockIdx.x * P;

  // adjoint of output o, stream s, at this lane's point of tile t (0 outside / for NULL);
  // read where used: the backward's register budget is tight
  // In-kernel seeds (value jets, J.seeds): the threads form the block's (tile, output, point) adjoints --
  // from gy, or from the loss terms (jet_common.hpp seed_gather / seed_finish: the operands are loaded
  // before the output layer's z-streams, the adjoint formed after them, so both loads share one latency;
  // that thread also counts the term's square) -- into LDS; the waves' square sums meet after one
  // barrier and thread 0 writes the block's row of J.seeds.lpart
  float* sseed = zred + 2 * 5 * 8;  // [t][o][c]
  constexpr bool kSeed1 = S == 1 && T * 48 <= G::THREADS;  // one element per thread (the value shapes)
  SeedOps sop{0.f, 0.f, 0.f, 0.f, -1};
  float sgy = 0.f;
  if constexpr (kSeed1) {
    if (J.seeds.nt) {
      const int i = threadIdx.x, t = i / 48, o = (i / 16) % 3, p = (tile0 + t) * 16 + (i & 15);
      if (i < T * 48 && t < cnt && p < N && o < dout) {
        const long e = (long)p * dout + o;
        if (gy)
          sgy = gy[e];
        else
          sop = seed_gather(J.seeds, jk, INSR_SEED_VALUE, e);
      }
    }
  }
  auto seed_stage = [&]() {
    if constexpr (S == 1) {
      if (J.seeds.nt) {
        float* swq = sseed + T * 48;  // [wave][INSR_SEED_MAX]
        float sq[INSR_SEED_MAX] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (kSeed1) {
          if (threadIdx.x < T * 48) sseed[threadIdx.x] = gy ? sgy : seed_finish(J.seeds, sop, sq);
        } else {
          for (int i = threadIdx.x; i < T * 48; i += G::THREADS) {
            const int t = i / 48, o = (i / 16) % 3, p = (tile0 + t) * 16 + (i & 15);
            float v = 0.f;
            if (t < cnt && p < N && o < dout) {
              const long e = (long)p * dout + o;
              v = gy ? gy[e] : seed_adjoint(J.seeds, jk, INSR_SEED_VALUE, e, true, sq);
            }
            sseed[i] = v;
          }
        }
#pragma unroll
        for (int q = 0; q < INSR_SEED_MAX; ++q) {
          float v = sq[q];
          for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
          if (lane == 0) swq[wave * INSR_SEED_MAX + q] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          floatx4 r = floatx4{0.f, 0.f, 0.f, 0.f};
          for (int w = 0; w < G::THREADS / 64; ++w)
#pragma unroll
            for (int q = 0; q < INSR_SEED_MAX; ++q) r[q] += swq[w * INSR_SEED_MAX + q];
          *reinterpret_cast<floatx4*>(J.seeds.lpart + (long)blockIdx.x * INSR_SEED_MAX) = r;
        }
      }
    }
  };
  auto adjoint = [&](int t, int s, int o) -> float {
    const int p = (tile0 + t) * 16 + c;
    if constexpr (S == 1)
      if (J.seeds.nt) return sseed[(t * 3 + o) * 16 + c];
    if (t >= cnt || p >= N) return 0.f;
    if (s == 0) return gy ? gy[(long)p * dout + o] : 0.f;
    if (LAP && s == S - 1) return glap ? glap[(long)p * dout + o] : 0.f;
    return gdy ? gdy[((long)p * dout + o) * din + (s - 1)] : 0.f;
  };

  auto load_sc = [&](int layer, floatx4(&s_)[T][RPW], floatx4(&c_)[T][RPW]) {
    floatx4 z[T][RPW];
    float amax = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float* base = act_base(act, layer, ntiles, tt(t), S, NT);
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        z[t][i] = *reinterpret_cast<const floatx4*>(base + ((rt0 + i) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(OMEGA * z[t][i][r]));
      }
    }
    const bool big = wave_any_big(amax);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < RPW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv, cv;
          if (big)
            sincosf(OMEGA * z[t][i][r], &sv, &cv);
          else
            sincos_fast(OMEGA * z[t][i][r], sv, cv);
          s_[t][i][r] = sv;
          c_[t][i][r] = cv;
        }
  };

  // ---- output layer (exact fp32 VALU) ----
  floatx4 sn[T][RPW], cs[T][RPW];
  load_sc(L, sn, cs);
  seed_stage();  // (the seeds' operands were loaded before load_sc's z-streams)
  const float* Wo = prm + out_off(din, W, L);
  const long wo_off = out_off(din, W, L);
  floatx4 hb[T][RPW][S];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < RPW; ++i)
#pragma unroll
      for (int s = 0; s < S; ++s) hb[t][i][s] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int o = 0; o < dout; ++o) {
    float ga[T][S];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int s = 0; s < S; ++s) ga[t][s] = adjoint(t, s, o);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int rt = rt0 + i;
      const floatx4 w4 = *reinterpret_cast<const floatx4*>(Wo + (o * W + 16 * rt + 4 * g));
      floatx4 acc4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float* baseL = act_base(act, L, ntiles, tt(t), S, NT);
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const floatx4 hs = h_stream<NT, S, LAP>(baseL, s, rt, lane, sn[t][i], cs[t][i]);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc4[r] = fmaf(ga[t][s], hs[r], acc4[r]);
            hb[t][i][s][r] = fmaf(w4[r], ga[t][s], hb[t][i][s][r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = sum16(acc4[r]);
        if (c == 0) mypart[wo_off + (long)o * W + 16 * rt + 4 * g + r] = v;
      }
    }
    if (wave == 0) {  // db_out[o]: every point counted once (lane group g == 0)
      float v = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t) v += (g == 0) ? ga[t][0] : 0.f;
      v = sum16(v);
      if (lane == 0) mypart[wo_off + (long)dout * W + o] = v;
    }
  }

  // ---- sine layers j = L .. 0 ----
  // KZ: the derivative z-streams of layer j-1 are loaded once (early, before the first
  // barrier of layer j) and serve both h_{j-1} and the sine reverse of layer j-1
#ifndef X6_KZ_MAX
#define X6_KZ_MAX 3  // measured: keeping more z-streams costs spills (LAP/GRAD at T = 2)
#endif
  constexpr bool KZ = S > 1 && T * RPW * (S - 1) <= X6_KZ_MAX;
  constexpr int ZK = KZ ? S - 1 : 1;  // streams 1 .. S-1 (zk[..][s - 1])
  floatx4 zk[KZ ? T : 1][KZ ? RPW : 1][ZK];
  auto load_zk = [&](int layer) {
    if constexpr (KZ) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float* base = act_base(act, layer, ntiles, tt(t), S, NT);
        const bool l0 = l0_rebuilt(layer, L);
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int s = 1; s < S; ++s) zk[t][i][s - 1] = load_zs<NT, S, LAP>(base, s, rt0 + i, lane, l0, prm, din);
      }
    }
  };
  load_zk(L);
  const u32x4* wsp = wsp_base(prm, din, dout, L, W);
  for (int j = L; j >= 0; --j) {
    INSR_STAMP(L - j, 0);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float* basej = act_base(act, j, ntiles, tt(t), S, NT);
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        if constexpr (KZ) {
          floatx4 zs[S];
          zs[0] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 1; s < S; ++s) zs[s] = zk[t][i][s - 1];
          sine_rev<S, LAP>(hb[t][i], zs, sn[t][i], cs[t][i]);
        } else {
          floatx4 zs[S];
#pragma unroll
          for (int s = 0; s < S; ++s)
            zs[s] = (s == 0) ? floatx4{0.f, 0.f, 0.f, 0.f}
                             : load_zs<NT, S, LAP>(basej, s, rt0 + i, lane, l0_rebuilt(j, L), prm, din);
          sine_rev<S, LAP>(hb[t][i], zs, sn[t][i], cs[t][i]);
        }
      }
    }
    const long boff = (j == 0) ? (long)W * din : hidden_off(din, W, j) + (long)W * W;
#pragma unroll
    for (int i = 0; i < RPW; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) v += hb[t][i][0][r];
        v = sum16(v);
        if (c == 0) mypart[boff + 16 * (rt0 + i) + 4 * g + r] = v;
      }
    if (j == 0) {
#pragma unroll
      for (int i = 0; i < RPW; ++i)
        for (int k = 0; k < din; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const int p = (tile0 + t) * 16 + c;
              const float xk = (t < cnt && p < N) ? x[(long)p * din + k] : 0.f;
              v = fmaf(hb[t][i][0][r], xk, v);
              if (k < NTAN) v += hb[t][i][1 + k][r];
            }
            v = sum16(v);
            if (c == 0) mypart[(long)(16 * (rt0 + i) + 4 * g + r) * din + k] = v;
          }
      break;
    }
    INSR_STAMP(L - j, 1);
    if constexpr (NQ == 4) {  // this wave's max |z̄_j| over the block's tiles (read after the group barrier)
      float mv = 0.f, mt = 0.f, ml = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int s = 0; s < S; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (LAP && s == S - 1)
                ml = fmaxf(ml, fabsf(hb[t][i][s][r]));
              else if (s == 0)
                mv = fmaxf(mv, fabsf(hb[t][i][s][r]));
              else
                mt = fmaxf(mt, fabsf(hb[t][i][s][r]));
            }
      mv = wave_max(mv);
      if constexpr (S > 1) mt = wave_max(mt);
      if constexpr (LAP) ml = wave_max(ml);
      if (lane == 0) {  // two slots: layer j - 1 writes the other
        zred[((j & 1) * 5) * 8 + wave] = mv;
        zred[((j & 1) * 5 + 1) * 8 + wave] = ml;
        zred[((j & 1) * 5 + 3) * 8 + wave] = mt;
      }
    }
    // A operand of the propagation: W^T rows m = 16 rt + c, k = n = 32 kc + 8 g + jj, from the
    // pre-split planes (issued here, in flight during the dW phase).  Several stream groups:
    // re-read per group (L2 hits) instead of holding the fragments across groups
    FragQ<NQ> wt[RPW][KC];
    if constexpr (NG == 1 && !PM) {  // (PM streams them one K chunk ahead of the propagation)
#pragma unroll
      for (int i = 0; i < RPW; ++i)
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) wt[i][kc] = wsp_frag<NQ, NT>(wsp, L, 1, j, rt0 + i, kc, lane);
    }
    floatx4 snp[T][RPW], csp[T][RPW];
    load_sc(j - 1, snp, csp);
    load_zk(j - 1);
    if constexpr (NQ == 4 && S > 1) {  // this wave's bounds of h_{j-1}'s Laplacian (w |q| + w^2 sum t^2)
      float hl = 0.f, htb = 0.f;       // and tangent streams (w |t|)
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float* basep = act_base(act, j - 1, ntiles, tt(t), S, NT);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          floatx4 zd[S - 1];
#pragma unroll
          for (int s = 1; s < S; ++s) {
            if constexpr (KZ)
              zd[s - 1] = zk[t][i][s - 1];
            else
              zd[s - 1] = load_zs<NT, S, LAP>(basep, s, rt0 + i, lane, l0_rebuilt(j - 1, L), prm, din);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float t2 = 0.f;
#pragma unroll
            for (int k = 0; k < NTAN; ++k) {
              t2 = fmaf(zd[k][r], zd[k][r], t2);
              htb = fmaxf(htb, fabsf(zd[k][r]));
            }
            if constexpr (LAP) hl = fmaxf(hl, fmaf(OMEGA, fabsf(zd[S - 2][r]), OMEGA2 * t2));
          }
        }
      }
      if constexpr (LAP) hl = wave_max(hl);
      htb = wave_max(htb) * OMEGA;
      if (lane == 0) {
        zred[((j & 1) * 5 + 2) * 8 + wave] = hl;
        zred[((j & 1) * 5 + 4) * 8 + wave] = htb;
      }
    }
    floatx4 dacc[RPW][NT];
#pragma unroll
    for (int i = 0; i < RPW; ++i)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) dacc[i][ct] = floatx4{0.f, 0.f, 0.f, 0.f};
    floatx4 nh[T][RPW][S];
    // NQ = 4: the block's adjoint scale 2^e and its inverse; h_{j-1}'s Laplacian stream x hll = 2^eh,
    // the Laplacian adjoint x zll = 2^-eh more (e maps max(|z̄|, |z̄_lap| 2^-eh) into [2^14, 2^15))
    float zsc = 1.f, zun = 1.f, zll = 1.f, hll = 1.f, ztl = 1.f, htl = 1.f;
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      const int s0 = gi * SG;
      INSR_STAMP(L - j, 2);
      __syncthreads();  // the previous group's / layer's LDS readers are done
      INSR_STAMP(L - j, 3);
      if constexpr (NQ == 4) {
        if (gi == 0) {
          // h's tangent streams: unscaled while their bound stays below 2^15 (the common case); else
          // x 2^eht, and the z̄ tangent streams x 2^-eht (every dW product keeps the block's 2^e)
          const float* zr = zred + (j & 1) * 5 * 8;
          float mv = zr[0], ml = zr[8], mh = zr[16], mt = zr[24], mht = zr[32];
#pragma unroll
          for (int w = 1; w < G::WV; ++w) {
            mv = fmaxf(mv, zr[w]);
            ml = fmaxf(ml, zr[8 + w]);
            mh = fmaxf(mh, zr[16 + w]);
            mt = fmaxf(mt, zr[24 + w]);
            mht = fmaxf(mht, zr[32 + w]);
          }
          if constexpr (LAP) {
            hll = ldexpf(1.f, f16_exp_for(mh));
            zll = 1.f / hll;
          }
          if constexpr (S > 1) {
            htl = ldexpf(1.f, mht >= 32768.f ? f16_exp_for(mht) : 0);
            ztl = 1.f / htl;
          }
          const int e = f16_exp_for(fmaxf(mv, fmaxf(mt * ztl, ml * zll)));
          zsc = ldexpf(1.f, e);
          zun = ldexpf(1.f, -e);
        }
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float* basep = act_base(act, j - 1, ntiles, tt(t), S, NT);
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int sl = 0; sl < SG; ++sl) {
            const int s = s0 + sl;
            const int u = t * SG + sl;
            const int col = 16 * (rt0 + i) + 4 * g;
            const bool lq = NQ == 4 && LAP && s == S - 1;  // the fp16 Laplacian-stream scales
            const bool tq = NQ == 4 && s > 0 && !lq;        // ... and the tangent streams'
            const float fl = lq ? zll : (tq ? ztl : 1.f);   // after zsc: each factor within fp32's range
            lds_put4<NQ, ZPLANE>(Z + u * ZSET + c * LDB + col, (hb[t][i][s][0] * zsc) * fl,
                                 (hb[t][i][s][1] * zsc) * fl, (hb[t][i][s][2] * zsc) * fl,
                                 (hb[t][i][s][3] * zsc) * fl);
            floatx4 hs;
            if constexpr (KZ) {
              hs = h_from_regs<S, LAP>(s, zk[t][i], snp[t][i], csp[t][i]);
            } else {
              hs = h_stream<NT, S, LAP>(basep, s, rt0 + i, lane, snp[t][i], csp[t][i], l0_rebuilt(j - 1, L), prm,
                                        din);
            }
            if (lq) hs *= hll;
            if (tq) hs *= htl;
            if constexpr (PM)
              lds_put4<NQ, ZPLANE>(H + u * HSET + c * LDB + col, hs[0], hs[1], hs[2], hs[3]);
            else
              put_neuron_major<NQ, HPLANE>(H + u * HSET, hs, col, c);
          }
      }
      INSR_STAMP(L - j, 4);
      __syncthreads();
      INSR_STAMP(L - j, 5);
      if constexpr (PM) {
        // the propagation's first W^T fragment: its L2 latency runs under the dW MFMAs
        FragQ<NQ> wn = wsp_frag<NQ, NT>(wsp, L, 1, j, rt0, 0, lane);
        // dW_j: wave (ra, cb) = (wave >> 1, wave & 1) owns row tiles 2 ra, 2 ra + 1 (A: column reads of
        // the Z sets) x column tiles 4 cb .. 4 cb + 3 (B: the same transpose reads of the H sets; lane c
        // receives neuron c at the chunk's 8 points, the K placement of A) -- 6 fragment reads per 8
        // MFMA triples (a wave owning one row tile x all 8 column tiles: 9).  This loop and the propagation
        // below are jet_fb.hpp bwd_layer's with tiles for streams: a change to one belongs in the other
        // (why they are two copies and not one function: DESIGN.md section 14)
        const int ra = wave >> 1, cb = wave & 1;
        floatx4 dq[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) dq[q] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (2 * ch >= cnt) break;  // unused tile slots of a balanced block
          const int u = 2 * ch + (g >> 1);
          const bool live = u < cnt;
          const int p0 = 8 * (g & 1);
          const int lo_ = (p0 + (c >> 2)) * LDB + 4 * (c & 3);
          FragQ<NQ> af[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const FragQ<NQ> a = lds_frag_tr<NQ, ZPLANE, LDB>(Z + (live ? u : 0) * ZSET + lo_ + 16 * (2 * ra + i), live);
#pragma unroll
            for (int q = 0; q < 2; ++q) af[i].q[q] = a.q[q];  // plane by plane (lds_frag_tr)
          }
          // the next column tile's B fragment is issued before this one's MFMAs
          auto bfrag = [&](int q4) __attribute__((always_inline)) {
            return lds_frag_tr<NQ, ZPLANE, LDB>(H + (live ? u : 0) * HSET + lo_ + 16 * (4 * cb + q4));
          };
          FragQ<NQ> bf = bfrag(0);
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            FragQ<NQ> bn;
            if (q4 < 3) bn = bfrag(q4 + 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) dq[4 * i + q4] = mfma_q<NQ>(af[i], bf, dq[4 * i + q4]);
            X6_SCHED_FENCE();
            if (q4 < 3) bf = bn;
          }
        }
        {  // this wave's 2 x 4 tiles of dW_j: store now (frees the accumulators)
          float* dW = mypart + hidden_off(din, W, j);
#pragma unroll
          for (int q = 0; q < NT; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              dW[(16 * (2 * ra + q / 4) + 4 * g + r) * W + 16 * (4 * cb + q % 4) + c] = dq[q][r] * zun;
        }
        INSR_STAMP(L - j, 6);
        // propagation (an unused slot of a balanced block holds zero adjoints in Z: its products are
        // zeros).  W^T one K chunk ahead; the next (K chunk, tile) B fragment before this one's MFMAs
#pragma unroll
        for (int t = 0; t < T; ++t) nh[t][0][0] = floatx4{0.f, 0.f, 0.f, 0.f};
        FragQ<NQ> pb = lds_frag<NQ, ZPLANE>(Z + c * LDB + 8 * g);
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const FragQ<NQ> wc = wn;
          if (kc + 1 < KC) wn = wsp_frag<NQ, NT>(wsp, L, 1, j, rt0, kc + 1, lane);
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int nk = t + 1 < T ? kc : kc + 1, nt = t + 1 < T ? t + 1 : 0;
            FragQ<NQ> pn;
            if (nk < KC) pn = lds_frag<NQ, ZPLANE>(Z + nt * ZSET + c * LDB + 32 * nk + 8 * g);
            nh[t][0][0] = mfma_q<NQ>(wc, pb, nh[t][0][0]);
            X6_SCHED_FENCE();
            if (nk < KC) pb = pn;
          }
        }
      } else {
      // dW_j rows n = 16 rt + c (A), columns m (B); K = sets x 16 points
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (2 * ch >= cnt * SG) break;  // unused tile slots of a balanced block (sets t SG + sl)
        const int u = 2 * ch + (g >> 1);
        const bool live = u < cnt * SG;
        const int p0 = 8 * (g & 1);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          // column reads of the point-major Z image: this wave's 16 neurons at the chunk's 8 points
          const FragQ<NQ> a = lds_frag_tr<NQ, ZPLANE, LDB>(
              Z + (live ? u : 0) * ZSET + (p0 + (c >> 2)) * LDB + 16 * (rt0 + i) + 4 * (c & 3), live);
          FragQ<NQ> af;
#pragma unroll
          for (int q = 0; q < np_of<NQ>(); ++q) af.q[q] = a.q[q];  // plane by plane (lds_frag_tr)
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) {
            const FragQ<NQ> bf = lds_frag<NQ, HPLANE>(H + (live ? u : 0) * HSET + (16 * ct + c) * 16 + p0);
            dacc[i][ct] = mfma_q<NQ>(af, bf, dacc[i][ct]);
            X6_SCHED_FENCE();
          }
        }
      }
      if constexpr (NG == 1) {  // dW_j rows of this wave: store now (frees the accumulators)
        float* dW = mypart + hidden_off(din, W, j);
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) dW[(16 * (rt0 + i) + 4 * g + r) * W + 16 * ct + c] = dacc[i][ct][r] * zun;
      }
      INSR_STAMP(L - j, 6);
      if constexpr (NG > 1) {
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) wt[i][kc] = wsp_frag<NQ, NT>(wsp, L, 1, j, rt0 + i, kc, lane);
      }
      // propagation of this group's streams (an unused slot of a balanced block keeps zero
      // adjoints: its bias / first-layer sums must add nothing)
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int sl = 0; sl < SG; ++sl) {
          const int s = s0 + sl;
          const int u = t * SG + sl;
#pragma unroll
          for (int i = 0; i < RPW; ++i) nh[t][i][s] = floatx4{0.f, 0.f, 0.f, 0.f};
          if (t >= cnt) continue;
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) {
            const FragQ<NQ> bf = lds_frag<NQ, ZPLANE>(Z + u * ZSET + c * LDB + 32 * kc + 8 * g);
#pragma unroll
            for (int i = 0; i < RPW; ++i) nh[t][i][s] = mfma_q<NQ>(wt[i][kc], bf, nh[t][i][s]);
            X6_SCHED_FENCE();
          }
        }
      }  // !PM
    }
    INSR_STAMP(L - j, 7);
    if constexpr (NG > 1) {  // dW_j rows of this wave
      float* dW = mypart + hidden_off(din, W, j);
#pragma unroll
      for (int i = 0; i < RPW; ++i)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) dW[(16 * (rt0 + i) + 4 * g + r) * W + 16 * ct + c] = dacc[i][ct][r] * zun;
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        sn[t][i] = snp[t][i];
        cs[t][i] = csp[t][i];
#pragma unroll
        for (int s = 0; s < S; ++s)
          hb[t][i][s] = (NQ == 4) ? (nh[t][i][s] * zun) *
                                        (((LAP && s == S - 1) ? hll : (s > 0 ? htl : 1.f)) / kF16WScale)
                                  : nh[t][i][s];
      }
  }
}

template <int NQ, int NT, int S, bool LAP, int T>
int launch_bwd_x6_t(const BwdJobsX6* J, int din, int dout, int L, const float* prm, float* part, long P,
                    hipStream_t st) {
  constexpr size_t lds = bwd_x6_lds_bytes<NQ, NT, S, T>();
  if constexpr (lds > kLdsMax || NT > 8) {
    return INSR_EINVAL;
  } else {
    static const bool attr_set = ((void)hipFuncSetAttribute((const void*)jet_bwd_x6<NQ, NT, S, LAP, T>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), true);  // once per instantiation (thread-safe static init)
    (void)attr_set;
    if (!J) {  // occupancy query (split_tiles): resident blocks per CU
      int occ = 0;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)jet_bwd_x6<NQ, NT, S, LAP, T>, X6Geo<NT>::THREADS, lds);
      return occ;
    }
    if (J->njobs < 1 || J->njobs > kBwdJobs) return INSR_EINVAL;
    const int nb = J->first[J->njobs];
    if (nb <= 0) return 0;
    hipLaunchKernelGGL((jet_bwd_x6<NQ, NT, S, LAP, T>), dim3(nb), dim3(X6Geo<NT>::THREADS), lds, st, *J, din, dout, L,
                       prm, part, P);
    return (int)hipGetLastError();
  }
}

}  // namespace insr
