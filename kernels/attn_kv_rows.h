// attn_kv_rows.h — what the KV-cache attention kernels share: the cache's row formats, the split
// bookkeeping's constants, the host checks' helpers and the launch of the splits' merge.
// Included by attn_kv.hip (the VALU forms, 1 .. 16 query rows) and attn_kv_mfma.hip (the MFMA form, any
// row count); the formats are documented in attn_kv.hip's header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kfkv {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kSplitKeys = 256;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kFp8Max = 448.f;  // largest finite e4m3fn value (code 0x7E)

// ---- row formats -------------------------------------------------------------------------------
// What a cache row is made of. Elem: the unit of the cache strides. Vec: one lane's load, 8 elements.
// kStrideAlign: what every cache stride must be a multiple of, in Elem (16 B either way). unroll(R): keys
// per lane group and block step, loaded one step ahead. kScaled: a row has an fp32 scale next to it.
// to_bf16: the 8 elements as 8 bf16 (exact for both formats), what the MFMA form stages into LDS.
struct Bf16Rows {
  typedef __bf16 Elem;
  typedef u32x4 Vec;
  static constexpr bool kScaled = false;
  static constexpr int kStrideAlign = 8;
  static constexpr int unroll(int) { return 2; }
  static __device__ __forceinline__ void unpack8(const Vec& w, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ u32x4 to_bf16(const Vec& w) { return w; }
};

struct Fp8Rows {
  typedef uint8_t Elem;
  typedef u32x2 Vec;
  static constexpr bool kScaled = true;
  static constexpr int kStrideAlign = 16;
  // A lane's load is 8 B, half of bf16's: twice bf16's unroll keeps the same bytes in flight where the
  // kernel is a KV stream (up to 4 row slots); at 8 row slots the VALU sets the time and the registers
  // go to the accumulators.
  static constexpr int unroll(int R) { return R >= 8 ? 2 : 4; }
  // 8 e4m3 codes (memory order: byte 0 first) -> fp32
  static __device__ __forceinline__ void unpack8(const Vec& w, float* f) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
      f[4 * i] = lo[0];
      f[4 * i + 1] = lo[1];
      f[4 * i + 2] = hi[0];
      f[4 * i + 3] = hi[1];
    }
  }
  // an e4m3 value has 4 significant bits and an exponent inside bf16's: the upper half of its fp32 is it
  static __device__ __forceinline__ u32x4 to_bf16(const Vec& w) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
      r[2 * i] = (__float_as_uint(lo[0]) >> 16) | (__float_as_uint(lo[1]) & 0xffff0000u);
      r[2 * i + 1] = (__float_as_uint(hi[0]) >> 16) | (__float_as_uint(hi[1]) & 0xffff0000u);
    }
    return r;
  }
};

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// Grouped-query attention: G query heads share one K / V head (query head h reads K / V head h / G). The
// kernels take G in {1, 2, 4, 8, 16} as its log2; -1 for every other value.
inline int group_log2(int G) { return G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : -1; }

// attn_kv_combine<D> (attn_kv.hip) on stream s: the splits' (m, l, o[D]) fp32 records, workspace layout
// [B][H][Tq][nsplit][2] then [B][H][Tq][nsplit][D], merged into bf16 rows o (strides ob, ot, oh) and the
// optional lse [B][Tq][H]. D: 64 or 128; Tq <= 65535 (it is gridDim.z). lg > 0: the grouped form
// (attn_kv_combine_gqa<D>): H is Hkv, Tq the T * G flattened rows r = t * G + g with G = 1 << lg, o's h stride
// runs over the Hkv * G query heads and lse is [B][T][Hkv * G].
hipError_t launch_kv_combine(int D, const float* ws, __bf16* o, float* lse, int B, int H, int Tq, int nsplit,
                             long long ob, long long ot, long long oh, hipStream_t s, int lg = 0);

}  // namespace kfkv
