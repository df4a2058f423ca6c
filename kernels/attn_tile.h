// attn_tile.h — the pieces the MFMA attention kernels share (attention_bf16.hip: flash forward and
// backward; attn_kv_mfma.hip: query tiles over the KV cache): the swizzled LDS image of a bf16 tile, its
// row and transposed reads, the 32x32x16 MFMA, the bf16 pair conversion and range-checked buffer loads.
// Lane maps: attention_bf16.hip's header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kfa {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int D>
__device__ __forceinline__ int swz(int row, int ch) {
  if constexpr (D == 128) {
    return ch ^ (((row & 3) << 2) | ((row >> 2) & 3));
  } else {
    const int x = (row >> 1) & 7;
    return ch ^ (((x & 1) << 2) | (x >> 1));
  }
}

// byte offset of 16-B chunk ch of row `row` in an image of D-element bf16 rows
template <int D>
__device__ __forceinline__ int img_off(int row, int ch) {
  return row * (D * 2) + (swz<D>(row, ch) << 4);
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// v_exp_f32 as is: the libm exp2f wraps it in a denormal range reduction (v_cmp, v_cndmask, v_ldexp
// per call) that softmax does not need — a result below 2^-126 is 0 for a probability
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ uint32_t pack2(float x, float y) {
  const bf16x2 v = __builtin_convertvector((f32x2){x, y}, bf16x2);
  return __builtin_bit_cast(uint32_t, v);
}

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ds_read_b64_tr_b16 at an LDS byte offset: 4 consecutive rows x 16 columns per 16-lane group,
// lane i of the group receives column i (row q in element q)
__device__ __forceinline__ s16x4 tr_read(const char* smem, int byte_off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + byte_off));
}

__device__ __forceinline__ bf16x8 join(s16x4 lo, s16x4 hi) {
  const short __attribute__((ext_vector_type(8))) v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 lds_row(const char* smem, int byte_off) {
  return *reinterpret_cast<const bf16x8*>(smem + byte_off);
}

__device__ __forceinline__ u32x4 gload16(const __bf16* p) { return *reinterpret_cast<const u32x4*>(p); }

// Raw buffer operations over one slice whose range ends after `bytes`: an access past it reads as zero
// (or is dropped) in the address unit, so row guards cost no branch. 32-bit offsets: the host keeps
// every slice below 2^31 bytes.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slice_rsrc(const void* base, long long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, int byte_off, int soff = 0) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, soff, 0));
}

}  // namespace kfa
