// swiglu_bf16.hip — the SwiGLU gate as its own elementwise pass (rows above the weight-streaming GEMM's 16, and
// training): z [rows][2F] interleaved (column 2j gate g, 2j + 1 up u; ops/swiglu.py states the rule) ->
//   forward   h[j]      = silu(g) * u,                 silu(g) = g * s, s = 1 / (1 + exp(-g))
//   backward  dz[2j]    = dh * u * s * (1 + g * (1 - s))
//             dz[2j+1]  = dh * silu(g)
// bf16 I/O, fp32 arithmetic, one rounding per output. Memory-bound and nothing is shared between lanes, so
// there is no LDS: a lane takes 8 outputs, i.e. two 16-B loads of z (4 pairs each) and one 16-B store of h
// forward; one 16-B load of dh, two of z and two 16-B stores of dz backward. That vector path needs F % 8 == 0,
// row strides % 8 == 0 and 16-B aligned bases; anything else takes the scalar path, one pair per thread. Rows
// are addressed by their strides, so a view with padded rows works and its padding is never touched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float sigmoidf(float g) { return 1.f / (1.f + __expf(-g)); }

__global__ __launch_bounds__(256) void swiglu_fwd_vec(const __bf16* __restrict__ z, __bf16* __restrict__ h,
                                                     long long units, int upr, long long ldz, long long ldh) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= units) return;
  const long long row = i / upr;
  const int c = (int)(i - row * upr);  // 8 outputs from column 8 c
  const bf16x8* zp = reinterpret_cast<const bf16x8*>(z + row * ldz + 16LL * c);
  const bf16x8 a = __builtin_nontemporal_load(zp), b = __builtin_nontemporal_load(zp + 1);
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float g0 = (float)a[2 * e], g1 = (float)b[2 * e];
    o[e] = (__bf16)(g0 * sigmoidf(g0) * (float)a[2 * e + 1]);
    o[4 + e] = (__bf16)(g1 * sigmoidf(g1) * (float)b[2 * e + 1]);
  }
  *reinterpret_cast<bf16x8*>(h + row * ldh + 8LL * c) = o;
}

__global__ __launch_bounds__(256) void swiglu_fwd_scalar(const __bf16* __restrict__ z, __bf16* __restrict__ h,
                                                        long long n, int F, long long ldz, long long ldh) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / F;
  const int j = (int)(i - row * F);
  const float g = (float)z[row * ldz + 2 * j], u = (float)z[row * ldz + 2 * j + 1];
  h[row * ldh + j] = (__bf16)(g * sigmoidf(g) * u);
}

__device__ __forceinline__ void glu_grad(float d, float g, float u, __bf16& dg, __bf16& du) {
  const float s = sigmoidf(g);
  dg = (__bf16)(d * u * s * (1.f + g * (1.f - s)));
  du = (__bf16)(d * (g * s));
}

__global__ __launch_bounds__(256) void swiglu_bwd_vec(const __bf16* __restrict__ dh, const __bf16* __restrict__ z,
                                                     __bf16* __restrict__ dz, long long units, int upr, long long lddh,
                                                     long long ldz, long long lddz) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= units) return;
  const long long row = i / upr;
  const int c = (int)(i - row * upr);
  const bf16x8 d = *reinterpret_cast<const bf16x8*>(dh + row * lddh + 8LL * c);
  const bf16x8* zp = reinterpret_cast<const bf16x8*>(z + row * ldz + 16LL * c);
  const bf16x8 a = zp[0], b = zp[1];
  bf16x8 oa, ob;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    __bf16 dg, du;
    glu_grad((float)d[e], (float)a[2 * e], (float)a[2 * e + 1], dg, du);
    oa[2 * e] = dg, oa[2 * e + 1] = du;
    glu_grad((float)d[4 + e], (float)b[2 * e], (float)b[2 * e + 1], dg, du);
    ob[2 * e] = dg, ob[2 * e + 1] = du;
  }
  bf16x8* op = reinterpret_cast<bf16x8*>(dz + row * lddz + 16LL * c);
  op[0] = oa;
  op[1] = ob;
}

__global__ __launch_bounds__(256) void swiglu_bwd_scalar(const __bf16* __restrict__ dh, const __bf16* __restrict__ z,
                                                        __bf16* __restrict__ dz, long long n, int F, long long lddh,
                                                        long long ldz, long long lddz) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / F;
  const int j = (int)(i - row * F);
  __bf16 dg, du;
  glu_grad((float)dh[row * lddh + j], (float)z[row * ldz + 2 * j], (float)z[row * ldz + 2 * j + 1], dg, du);
  dz[row * lddz + 2 * j] = dg;
  dz[row * lddz + 2 * j + 1] = du;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int finish() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

extern "C" int kfamd_swiglu_fwd_bf16(const void* z, void* h, long long rows, int F, long long ldz, long long ldh,
                                     void* stream) {
  if (!z || !h || rows < 1 || F < 1 || ldz < 2LL * F || ldh < F) return KFAMD_EINVAL;
  const long long n = rows * F;
  if ((n + 255) / 256 > 0x7fffffffLL) return KFAMD_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const __bf16* zp = static_cast<const __bf16*>(z);
  __bf16* hp = static_cast<__bf16*>(h);
  if (F % 8 == 0 && ldz % 8 == 0 && ldh % 8 == 0 && al16(z) && al16(h)) {
    const long long units = n / 8;
    hipLaunchKernelGGL(swiglu_fwd_vec, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, zp, hp, units, F / 8, ldz,
                       ldh);
  } else {
    hipLaunchKernelGGL(swiglu_fwd_scalar, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, zp, hp, n, F, ldz, ldh);
  }
  return finish();
}

extern "C" int kfamd_swiglu_bwd_bf16(const void* dh, const void* z, void* dz, long long rows, int F, long long lddh,
                                     long long ldz, long long lddz, void* stream) {
  if (!dh || !z || !dz || rows < 1 || F < 1 || lddh < F || ldz < 2LL * F || lddz < 2LL * F) return KFAMD_EINVAL;
  const long long n = rows * F;
  if ((n + 255) / 256 > 0x7fffffffLL) return KFAMD_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const __bf16* dp = static_cast<const __bf16*>(dh);
  const __bf16* zp = static_cast<const __bf16*>(z);
  __bf16* op = static_cast<__bf16*>(dz);
  if (F % 8 == 0 && lddh % 8 == 0 && ldz % 8 == 0 && lddz % 8 == 0 && al16(dh) && al16(z) && al16(dz)) {
    const long long units = n / 8;
    hipLaunchKernelGGL(swiglu_bwd_vec, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, dp, zp, op, units, F / 8,
                       lddh, ldz, lddz);
  } else {
    hipLaunchKernelGGL(swiglu_bwd_scalar, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dp, zp, op, n, F, lddh, ldz,
                       lddz);
  }
  return finish();
}
