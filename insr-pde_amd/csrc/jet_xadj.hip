// jet_xadj.hip -- the coordinate adjoint of the reverse jets (jet_xadj.hpp) and its C ABI
// (include/insr_siren.h insr_siren_jet_bwd_x*): exact fp32, widths 32 / 64 / 128 / 256, value,
// gradient and Laplacian jets of d_in 1..3, d_out 1..3.
#include "jet_xadj.hpp"

namespace insr {
namespace {

int xadj_nt(int width) {
  if (width == 32) return 2;
  if (width == 64) return 4;
  if (width == 128) return 8;
  if (width == 256) return 16;
  return -1;
}

// streams of the call's jet mode (its precision and knob bits are not read), -1: not a jet mode
int xadj_streams(int din, int mode) {
  const int jm = mode & INSR_MODE_MASK;
  if (jm == INSR_MODE_VALUE) return 1;
  if (jm == INSR_MODE_GRAD) return 1 + din;
  if (jm == INSR_MODE_LAP) return 2 + din;
  return -1;
}

// points per call: 16 * ceil(n / 16) stays an int in the kernel's point index
constexpr long kXadjMaxPoints = 0x7fffffffL - 15;

// 0, or why not: INSR_EINVAL (shape / mode) / INSR_EWIDTH (a width outside the compiled set)
int xadj_shape_rc(int din, int dout, int L, int width, int mode) {
  if (din < 1 || din > 3 || dout < 1 || dout > 3 || L < 0 || L > 64 || width < 1) return INSR_EINVAL;
  if (xadj_streams(din, mode) < 0) return INSR_EINVAL;
  return xadj_nt(width) < 0 ? INSR_EWIDTH : 0;
}

template <int NT>
int dispatch_nt(int S, bool LAP, int N, int din, int dout, int L, const float* prm, const float* act, const float* gy,
                const float* gdy, const float* glap, float* gx, hipStream_t st) {
  INSR_DISPATCH(NT, launch_bwd_x, N, din, dout, L, prm, act, gy, gdy, glap, gx, st)
}

int dispatch_bwd_x(int NT, int S, bool LAP, int N, int din, int dout, int L, const float* prm, const float* act,
                   const float* gy, const float* gdy, const float* glap, float* gx, hipStream_t st) {
  switch (NT) {
    case 2: return dispatch_nt<2>(S, LAP, N, din, dout, L, prm, act, gy, gdy, glap, gx, st);
    case 4: return dispatch_nt<4>(S, LAP, N, din, dout, L, prm, act, gy, gdy, glap, gx, st);
    case 8: return dispatch_nt<8>(S, LAP, N, din, dout, L, prm, act, gy, gdy, glap, gx, st);
    case 16: return dispatch_nt<16>(S, LAP, N, din, dout, L, prm, act, gy, gdy, glap, gx, st);
    default: return INSR_EWIDTH;
  }
}

}  // namespace
}  // namespace insr

using namespace insr;

extern "C" {

int insr_siren_jet_bwd_x_supported(int din, int dout, int L, int W, int mode) {
  if (xadj_shape_rc(din, dout, L, W, mode) != 0) return 0;
  // a call whose backward is the recompute kernel saves no streams (its forward passes act = NULL): nothing
  // to read.  Every other forward leaves fp32 z-streams in the one layout of insr_jet_act_bytes / act_base.
  // (The path of such a call does not depend on the batch size; a mode the jets themselves refuse answers
  // a negative code: no forward, no streams.)
  const int path = insr_jet_bwd_path(16, din, dout, L, W, mode);
  return (path < 0 || path == 3) ? 0 : 1;
}

int insr_siren_jet_bwd_x(long n, int din, int dout, int L, int W, int mode, const float* params, const float* act,
                         const float* gy, const float* gdy, const float* glap, float* gx, void* stream) {
  if (const int rc = xadj_shape_rc(din, dout, L, W, mode)) return rc;
  if (n < 0 || n > kXadjMaxPoints) return INSR_EINVAL;
  if (n == 0) return 0;
  if (!params || !act || !gx) return INSR_EINVAL;
  const int jm = mode & INSR_MODE_MASK;
  if (jm == INSR_MODE_VALUE) gdy = nullptr;  // adjoints of streams the jet does not carry are not read
  if (jm != INSR_MODE_LAP) glap = nullptr;
  if (!gy && !gdy && !glap) return (int)hipMemsetAsync(gx, 0, (size_t)n * din * sizeof(float), (hipStream_t)stream);
  return dispatch_bwd_x(xadj_nt(W), xadj_streams(din, mode), jm == INSR_MODE_LAP, (int)n, din, dout, L, params, act, gy,
                        gdy, glap, gx, (hipStream_t)stream);
}

}  // extern "C"
