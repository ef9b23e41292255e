// mesh_sampler.hip -- volume- / area-weighted mesh points of one phase iteration in ONE launch.
//
// The reference draws its mesh points with a Categorical draw over the elements' measures and
// Dirichlet(1, 1, 1, 1) (tets) or sqrt-warped (triangles) barycentrics (elasticity/torchgp/
// sample_volume.py, sample_surface.py, as called at elasticity/model.py:200-207).  pde/mesh.py
// MeshSampler.sample restates that as ~12 torch launches: a float64 uniform, searchsorted on the
// cumulative table, a corner gather, a second draw, log / sum / divide, a broadcast multiply and a
// sum.  Here one thread draws one point:
//   element      u = u0 + u1 2^-24 in fp64 (two 24-bit uniforms: one of 48 bits),
//                elem = min(#{i : cdf[i] <= u}, k - 1)      (searchsorted(right=True) + clamp)
//   tets         e_i = -log(max(r_i, 1e-30)), bary = e / sum e          (4 more uniforms)
//   triangles    su = sqrt(r0), bary = (1 - su, su (1 - r1), su r1)     (2 more uniforms)
//   point        out = sum_i bary_i corner_i  (fp32)
// mesh_point() below is that deterministic half; two kernels feed it:
//   mesh_points_kernel   the caller's uniforms (insr_mesh_points: MeshSampler.sample(uniforms=...))
//   sample_mesh_kernel   the box sampler's device Philox stream (sampler.hip): value v = p m + j of
//                        the launch = Philox4x32-10(seed, base + v / 4)[v % 4] -> (bits >> 8) 2^-24,
//                        m = 6 (tets) or 4 (triangles); the launch advances state[0] by
//                        ceil(n m / 4) itself, by sample_boxes_kernel's ticket rule.  It consumes
//                        exactly the numbers an insr_sample_boxes launch of n m values in [0, 1)
//                        would, so a captured graph draws fresh points on every replay and a
//                        following box draw continues the stream where it would have.
// No LDS, no atomics besides the ticket.  The search is branch-free: ceil(log2 k) steps, the same
// for every lane, each one fp64 load from the table (which sits in L2) at a clamped index -- no
// lane ever reads outside cdf[0, k - 1) or corners[0, k).
#include "jet_common.hpp"
#include "philox.hpp"

namespace insr {

struct MeshPk {
  const double* cdf;
  const float* corners;
  long k;
  long top;   // first step of the search: 2^(ceil(log2 k) - 1), 0 when k == 1
  int vec;    // the corner table may be read with 16-byte (tets) / 8-byte (2-d triangles) loads
};

constexpr float kU24 = 5.9604644775390625e-8f;  // 2^-24

// uniforms per point: two for the element, four (tets) or two (triangles) for the barycentrics
constexpr int mesh_uniforms(int nc) { return nc == 4 ? 6 : 4; }

// #{i : cdf[i] <= u}, clamped to k - 1: the count over the first k - 1 entries (the last entry can
// only add the element the clamp takes away again).  A NaN u compares false: element 0.
__device__ __forceinline__ long mesh_element(const MeshPk& m, double u) {
  const long last = m.k - 1;
  long c = 0;
  for (long step = m.top; step > 0; step >>= 1) {
    const long j = c + step;                       // candidate count
    const long i = (j < last ? j : last) - 1;      // in [0, k - 2]: steps only run for k >= 2
    c = (j <= last && m.cdf[i] <= u) ? j : c;
  }
  return c;
}

// NC corners of DIM coordinates of element e into c[NC * DIM]
template <int NC, int DIM>
__device__ __forceinline__ void mesh_corners(const MeshPk& m, long e, float* c) {
  const float* src = m.corners + e * (NC * DIM);
  if constexpr (NC * DIM % 4 == 0) {  // tets: 48 bytes, 16-byte aligned with the table
    if (m.vec) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
      for (int q = 0; q < NC * DIM / 4; ++q) {
        const float4 v = s4[q];
        c[4 * q] = v.x, c[4 * q + 1] = v.y, c[4 * q + 2] = v.z, c[4 * q + 3] = v.w;
      }
      return;
    }
  } else if constexpr (NC * DIM % 2 == 0) {  // 2-d triangles: 24 bytes
    if (m.vec) {
      const float2* s2 = reinterpret_cast<const float2*>(src);
#pragma unroll
      for (int q = 0; q < NC * DIM / 2; ++q) {
        const float2 v = s2[q];
        c[2 * q] = v.x, c[2 * q + 1] = v.y;
      }
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < NC * DIM; ++q) c[q] = src[q];
}

// uniforms u[0 .. mesh_uniforms(NC)) -> point p of `out` (and its element)
template <int NC, int DIM>
__device__ __forceinline__ void mesh_point(const MeshPk& m, const float* u, long p, float* __restrict__ out,
                                           int* __restrict__ elem) {
  const double ue = (double)u[0] + (double)u[1] * 5.9604644775390625e-8;
  const long e = mesh_element(m, ue);
  float c[NC * DIM];
  mesh_corners<NC, DIM>(m, e, c);
  float b[NC];
  if constexpr (NC == 4) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b[i] = -logf(fmaxf(u[2 + i], 1e-30f));
      s += b[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = b[i] / s;
  } else {
    const float su = sqrtf(u[2]);
    b[0] = 1.0f - su;
    b[1] = su * (1.0f - u[3]);
    b[2] = su * u[3];
  }
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    float v = b[0] * c[j];
#pragma unroll
    for (int i = 1; i < NC; ++i) v += b[i] * c[i * DIM + j];
    out[p * DIM + j] = v;
  }
  if (elem) elem[p] = (int)e;
}

template <int NC, int DIM>
__global__ __launch_bounds__(kSampThreads) void mesh_points_kernel(const MeshPk m, const float* __restrict__ uniforms,
                                                                   long n, float* __restrict__ out,
                                                                   int* __restrict__ elem) {
  constexpr int M = mesh_uniforms(NC);
  const long p = (long)blockIdx.x * kSampThreads + threadIdx.x;
  if (p >= n) return;
  float u[M];
#pragma unroll
  for (int j = 0; j < M; ++j) u[j] = uniforms[p * M + j];
  mesh_point<NC, DIM>(m, u, p, out, elem);
}

// state[0] = stream position (Philox counter), state[1] (low 32 bits) = the launch's ticket
template <int NC, int DIM>
__global__ __launch_bounds__(kSampThreads) void sample_mesh_kernel(const MeshPk m, long n, float* __restrict__ out,
                                                                   int* __restrict__ elem, unsigned long long seed,
                                                                   unsigned long long* __restrict__ state) {
  constexpr int M = mesh_uniforms(NC);
  const unsigned long long base = state[0];
  const long p = (long)blockIdx.x * kSampThreads + threadIdx.x;
  if (p < n) {
    float u[M];
    if constexpr (M == 4) {  // values 4 p .. 4 p + 3: group p
      const uint4 r = philox4x32_10(seed, base + (unsigned long long)p);
      const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = (float)(w[j] >> 8) * kU24;
    } else {  // values 6 p .. 6 p + 5 start at word 0 or 2 of group 6 p / 4 and end in the next group
      const unsigned long long v0 = (unsigned long long)p * 6;  // first value of this point
      const uint4 r0 = philox4x32_10(seed, base + (v0 >> 2));
      const uint4 r1 = philox4x32_10(seed, base + (v0 >> 2) + 1ull);
      const bool odd = (v0 & 2ull) != 0;
      const unsigned w[6] = {odd ? r0.z : r0.x, odd ? r0.w : r0.y, odd ? r1.x : r0.z,
                             odd ? r1.y : r0.w, odd ? r1.z : r1.x, odd ? r1.w : r1.y};
#pragma unroll
      for (int j = 0; j < 6; ++j) u[j] = (float)(w[j] >> 8) * kU24;
    }
    mesh_point<NC, DIM>(m, u, p, out, elem);
  }
  __syncthreads();  // every thread of this block has read `base`
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(state + 1);
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {  // last block: every block has read `base`
      state[0] = base + (unsigned long long)((n * M + 3) / 4);
      atomicExch(ticket, 0u);
    }
  }
}

// Host half: every refusal comes before any launch.  Returns 0 and fills pk / nb, or INSR_EINVAL.
static int mesh_check(const InsrMesh* mesh, long n, const void* out, MeshPk* pk, long* nb) {
  if (!mesh || !mesh->cdf || !mesh->corners || !out) return INSR_EINVAL;
  if (mesh->nc != 3 && mesh->nc != 4) return INSR_EINVAL;
  if (mesh->dim != 2 && mesh->dim != 3) return INSR_EINVAL;
  if (mesh->nc == 4 && mesh->dim == 2) return INSR_EINVAL;
  if (mesh->k < 1 || mesh->k > 0x7fffffffL || n < 0) return INSR_EINVAL;  // elem is a 32-bit index
  *nb = (n + kSampThreads - 1) / kSampThreads;
  if (*nb > 0x7fffffffL) return INSR_EINVAL;
  pk->cdf = mesh->cdf;
  pk->corners = mesh->corners;
  pk->k = mesh->k;
  long top = 0;  // 2^(ceil(log2 k) - 1): the smallest power of two with 2 top >= k
  if (mesh->k > 1)
    for (top = 1; 2 * top < mesh->k; top *= 2) {}
  pk->top = top;
  const uintptr_t a = (uintptr_t)mesh->corners;
  pk->vec = mesh->nc == 4 ? (a % 16 == 0) : (mesh->dim == 2 && a % 8 == 0);
  return 0;
}

}  // namespace insr

using namespace insr;

extern "C" {

long insr_mesh_uniforms_per_point(int nc) { return nc == 4 ? 6 : nc == 3 ? 4 : INSR_EINVAL; }

int insr_mesh_points(const InsrMesh* mesh, const float* uniforms, long n, float* out, int* elem, void* stream) {
  MeshPk pk{};
  long nb = 0;
  if (!uniforms) return INSR_EINVAL;
  if (int rc = mesh_check(mesh, n, out, &pk, &nb)) return rc;
  if (n == 0) return 0;
  const dim3 grid((unsigned)nb), block(kSampThreads);
  hipStream_t st = (hipStream_t)stream;
  if (mesh->nc == 4)
    hipLaunchKernelGGL((mesh_points_kernel<4, 3>), grid, block, 0, st, pk, uniforms, n, out, elem);
  else if (mesh->dim == 3)
    hipLaunchKernelGGL((mesh_points_kernel<3, 3>), grid, block, 0, st, pk, uniforms, n, out, elem);
  else
    hipLaunchKernelGGL((mesh_points_kernel<3, 2>), grid, block, 0, st, pk, uniforms, n, out, elem);
  return (int)hipGetLastError();
}

int insr_sample_mesh(const InsrMesh* mesh, long n, float* out, int* elem, unsigned long long seed, void* state,
                     void* stream) {
  MeshPk pk{};
  long nb = 0;
  if (!state) return INSR_EINVAL;
  if (int rc = mesh_check(mesh, n, out, &pk, &nb)) return rc;
  if (n == 0) return 0;
  const dim3 grid((unsigned)nb), block(kSampThreads);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* s = (unsigned long long*)state;
  if (mesh->nc == 4)
    hipLaunchKernelGGL((sample_mesh_kernel<4, 3>), grid, block, 0, st, pk, n, out, elem, seed, s);
  else if (mesh->dim == 3)
    hipLaunchKernelGGL((sample_mesh_kernel<3, 3>), grid, block, 0, st, pk, n, out, elem, seed, s);
  else
    hipLaunchKernelGGL((sample_mesh_kernel<3, 2>), grid, block, 0, st, pk, n, out, elem, seed, s);
  return (int)hipGetLastError();
}

}  // extern "C"
