// jet_hess.hip -- the second-order (full Hessian) jets of jet_hess.hpp and their C ABI
// (include/insr_siren.h insr_siren_hess_*): exact fp32, d_in 2 / 3, widths 32 / 64 / 128.
#include "jet_hess.hpp"

namespace insr {
namespace {

int hess_nt(int width) {
  if (width == 32) return 2;
  if (width == 64) return 4;
  if (width == 128) return 8;
  return -1;  // 256: the planes of ten streams do not fit a CU's LDS in this dataflow
}

// points per call: 16 * ceil(n / 16) stays an int in the kernels' point index
constexpr long kHessMaxPoints = 0x7fffffffL - 15;

int hess_streams(int din) { return din == 2 ? HessGeo<2>::S : din == 3 ? HessGeo<3>::S : -1; }

// 0, or why not: INSR_EINVAL (shape) / INSR_EWIDTH (a width outside the compiled set)
int hess_shape_rc(int din, int dout, int L, int width) {
  if (din < 2 || din > 3 || dout < 1 || dout > 3 || L < 0 || L > 64 || width < 1) return INSR_EINVAL;
  return hess_nt(width) < 0 ? INSR_EWIDTH : 0;
}

#define INSR_HESS_DISPATCH(FN, ...)                     \
  switch (NT * 4 + din) {                               \
    case 2 * 4 + 2: return FN<2, 2>(__VA_ARGS__);       \
    case 2 * 4 + 3: return FN<2, 3>(__VA_ARGS__);       \
    case 4 * 4 + 2: return FN<4, 2>(__VA_ARGS__);       \
    case 4 * 4 + 3: return FN<4, 3>(__VA_ARGS__);       \
    case 8 * 4 + 2: return FN<8, 2>(__VA_ARGS__);       \
    case 8 * 4 + 3: return FN<8, 3>(__VA_ARGS__);       \
    default: return INSR_EINVAL;                        \
  }

int dispatch_fwd_hess(int NT, int din, const float* x, int N, int dout, int L, const float* prm, float* y, float* dy,
                      float* hess, float* act, hipStream_t st) {
  INSR_HESS_DISPATCH(launch_fwd_hess, x, N, dout, L, prm, y, dy, hess, act, st)
}

int dispatch_bwd_hess(int NT, int din, const float* x, int N, int dout, int L, const float* prm, const float* act,
                      const float* gy, const float* gdy, const float* gh, float* part, long P, hipStream_t st) {
  INSR_HESS_DISPATCH(launch_bwd_hess, x, N, dout, L, prm, act, gy, gdy, gh, part, P, st)
}

}  // namespace
}  // namespace insr

using namespace insr;

extern "C" {

int insr_siren_hess_supported(int din, int dout, int L, int W) { return hess_shape_rc(din, dout, L, W) == 0 ? 1 : 0; }

long insr_hess_act_bytes(long n, int din, int L, int W) {
  const int S = hess_streams(din);
  if (S < 0 || n < 0 || L < 0 || W < 1) return INSR_EINVAL;
  return (long)(L + 1) * act_tiles(n) * 16 * W * S * (long)sizeof(float);
}

int insr_hess_partial_blocks(long n, int din, int W) {
  if (hess_streams(din) < 0 || n < 0 || n > kHessMaxPoints || W < 1) return INSR_EINVAL;
  return (int)((n + 15) / 16);
}

long insr_hess_partial_bytes(long n, int din, int dout, int L, int W) {
  const int nb = insr_hess_partial_blocks(n, din, W);
  if (nb < 0) return nb;
  if (dout < 1 || L < 0) return INSR_EINVAL;
  return (long)nb * insr_jet_partial_stride(din, dout, L, W) * (long)sizeof(float);
}

int insr_siren_hess_fwd(const float* x, long n, int din, int dout, int L, int W, const float* params, float* y,
                        float* dy, float* hess, float* act, void* stream) {
  if (const int rc = hess_shape_rc(din, dout, L, W)) return rc;
  if (n < 0 || n > kHessMaxPoints) return INSR_EINVAL;
  if (n == 0) return 0;
  if (!x || !params || !y || !dy || !hess) return INSR_EINVAL;
  return dispatch_fwd_hess(hess_nt(W), din, x, (int)n, dout, L, params, y, dy, hess, act, (hipStream_t)stream);
}

int insr_siren_hess_bwd(const float* x, long n, int din, int dout, int L, int W, const float* params,
                        const float* act, const float* gy, const float* gdy, const float* ghess, float* partial,
                        void* stream) {
  if (const int rc = hess_shape_rc(din, dout, L, W)) return rc;
  if (n < 0 || n > kHessMaxPoints) return INSR_EINVAL;
  if (n == 0) return 0;
  if (!x || !params || !act || !partial) return INSR_EINVAL;
  return dispatch_bwd_hess(hess_nt(W), din, x, (int)n, dout, L, params, act, gy, gdy, ghess, partial,
                           insr_jet_partial_stride(din, dout, L, W), (hipStream_t)stream);
}

}  // extern "C"
