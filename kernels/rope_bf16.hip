// rope_bf16.hip — rotary position embeddings on a fused QKV activation: the standalone rotation and the
// rotate-and-append into the KV cache (bf16 and FP8), one launch each.
//
// The rule (kubeflow_rm_amd/ops/rope.py holds it in full): the table is fp32 [max_pos][D], row p =
// cos(p f_0 .. p f_{D/2-1}) | sin(same), built on the host; no kernel here calls sin or cos. Rotate-half
// pairing: for i < D/2 at position p, with c = table[p][i], s = table[p][D/2 + i],
//     y[i]       = x[i] c - x[i + D/2] s
//     y[i + D/2] = x[i + D/2] c + x[i] s
// on bf16 inputs widened to fp32, the two products and the add / subtract each rounded on their own, the
// result rounded once to bf16 (RNE). hipcc contracts a * b + c into an FMA by default, which rounds once
// where the rule (and torch's fp32 ops) round twice: rot2 below switches contraction off (v_mul_f32 x 4,
// v_sub_f32, v_add_f32), and with it the kernels equal the torch form bit for bit. The inverse (the
// backward) is the same map with s -> -s; the sign is multiplied into s, which is exact.
//
// Work split: the activation is [B][T][(Hq + 2 Hkv) D], q: Hq D | k: Hkv D | v: Hkv D (element strides qb,
// qt). One lane owns the two 16-byte pieces (j, j + D/16) of one head row, the 8 + 8 elements that the
// pairing couples: 2 x 16 B of x, 2 x 32 B of the table (the cos and the sin of the same 8 frequencies),
// 2 x 16 B stored. A head row is D/16 lanes (4 at D = 64, 8 at D = 128). No LDS, vector loads and stores
// only, nothing read by one lane is written by another.
//   rope_qkv<D>           rotates the Hq + Hkv q and k head rows in place, v untouched. Position of row
//                         (b, t): (pos ? pos[b] : 0) + t; a row at or beyond max_pos is left as it is and
//                         the table is not read for it.
//   kv_append_rope<D, F8> the whole append step of a rotary layer: position lens[b] + t read on the
//                         device; q and k head rows rotated in place; the rotated K row and the V row
//                         written to cache row lens[b] + t. The FP8 form quantises the bf16-ROUNDED rotated
//                         K (kv_append_fp8's arithmetic on it), so codes and scale are those of
//                         quantize_rows on the rotated activation; the row's amax is kfw::group_max over
//                         the D/16 lanes. Rows at or beyond the capacity are neither appended nor rotated
//                         (the early return is uniform over a head row's lanes). max_pos >= Tcap is
//                         checked on the host, so the table is never read out of range.
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): rope_qkv<D> 42 VGPRs,
// kv_append_rope<D, F8> 58, at both head dims and for both caches; scratch 0 for every instantiation (checked at
// build time: _build.NO_SCRATCH_TUS). The rotation compiles to v_pk_mul_f32 / v_pk_add_f32 and v_cvt_pk_bf16_f32,
// no v_fma / v_fmac outside the FP8 form's IEEE divisions.
// kv_append_rope<D, F8, true> (a ring-buffer cache: absolute position, slot position % Tcap): 58 VGPRs, scratch 0.
// kv_append_rope<D, F8, false, true> (a paged cache: page pt[b][p >> 8], row p & 255): 56 VGPRs, scratch 0.
// Measured (profiles/rope; the gpt-1b layer, B = 8, 16 heads, D = 128): at T = 1 the fused append costs what
// kv_append costs (11.3 against 10.8 us bf16, 12.6 against 12.8 FP8) and half of rope_qkv + kv_append; at T = 2048
// 72.9 us (bf16) and 78.2 (FP8) against 49.1 / 61.8 for the append alone and 99.4 / 106.1 for two launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "attn_kv_rows.h"
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

using namespace kfkv;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One pair of the rotation, without FMA contraction: four products and two sums, six roundings.
__device__ __forceinline__ void rot2(float a, float b, float c, float s, float& ya, float& yb) {
#pragma clang fp contract(off)
  const float ac = a * c;
  const float bs = b * s;
  const float bc = b * c;
  const float as = a * s;
  ya = ac - bs;
  yb = bc + as;
}

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {  // RNE
  return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)lo) |
         ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)hi) << 16);
}

// The lane's 8 + 8 elements (lo: elements 8 j .., hi: D/2 + 8 j ..) rotated by table row trow (already at
// the lane's 8 frequencies: cos at trow, sin at trow + D/2). Returns the rotated values rounded to bf16.
template <int D>
__device__ __forceinline__ void rotate16(u32x4& lo, u32x4& hi, const float* __restrict__ trow, float sign) {
  float a[8], b[8], c[8], s[8];
  Bf16Rows::unpack8(lo, a);
  Bf16Rows::unpack8(hi, b);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x4 cv = *reinterpret_cast<const f32x4*>(trow + 4 * i);
    const f32x4 sv = *reinterpret_cast<const f32x4*>(trow + D / 2 + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[4 * i + e] = cv[e];
      s[4 * i + e] = sv[e] * sign;  // +-1: exact
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float ya0, yb0, ya1, yb1;
    rot2(a[2 * i], b[2 * i], c[2 * i], s[2 * i], ya0, yb0);
    rot2(a[2 * i + 1], b[2 * i + 1], c[2 * i + 1], s[2 * i + 1], ya1, yb1);
    lo[i] = pack_bf16(ya0, ya1);
    hi[i] = pack_bf16(yb0, yb1);
  }
}

template <int D>
__global__ __launch_bounds__(256) void rope_qkv(__bf16* x, const float* __restrict__ table,
                                                const int* __restrict__ pos, int B, int T, int NH, int max_pos,
                                                long long qb, long long qt, float sign) {  // NH = Hq + Hkv
  constexpr int G = D / 16;
  const long long n = (long long)B * T * NH * G;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int j = (int)(r % G);
  r /= G;
  const int h = (int)(r % NH);
  r /= NH;
  const int t = (int)(r % T);
  const int b = (int)(r / T);
  const long long p = (long long)(pos ? pos[b] : 0) + t;
  if (p < 0 || p >= max_pos) return;  // no table row: the activation row stays as it is
  __bf16* row = x + b * qb + t * qt + (long long)h * D + j * 8;
  u32x4 lo = *reinterpret_cast<const u32x4*>(row);
  u32x4 hi = *reinterpret_cast<const u32x4*>(row + D / 2);
  rotate16<D>(lo, hi, table + p * D + j * 8, sign);
  *reinterpret_cast<u32x4*>(row) = lo;
  *reinterpret_cast<u32x4*>(row + D / 2) = hi;
}

struct AppendArgs {
  __bf16* qkv;
  void* kc;  // __bf16 or uint8_t (codes)
  void* vc;
  float* ks;  // F8 only, as ksb .. vsh
  float* vs;
  const int* lens;
  const float* table;
  int B, T, Hq, Hkv, Tcap;
  long long qb, qt, kb, kh, kt, vb, vh, vt, ksb, ksh, vsb, vsh;
};

// The ring form's arguments: one more field, in a type of its own so that the flat kernels' argument block (and with
// it their code) stays as it was.
struct RingAppendArgs : AppendArgs {
  int max_pos;  // the table's rows
};

// The paged form's arguments (the page rule: ops/decode.py): kb, vb, ksb, vsb are the page strides.
struct PagedAppendArgs : AppendArgs {
  const int* pt;  // device int32 [B][pts]: the page of positions 256 c .. 256 c + 255 of row b, -1 for none
  long long pts;
  int n_pages;
  int max_pos;  // the table's rows: a row's capacity may be rounded up past them
};

// 8 bf16-valued floats -> 8 e4m3 codes at the row's scale: kv_append_fp8's arithmetic (attn_kv.hip)
__device__ __forceinline__ u32x2 fp8_codes(const float* x, float scale) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] / scale, -kFp8Max), kFp8Max);
  u32x2 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i], y[4 * i + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i + 2], y[4 * i + 3], p, true);
    w[i] = (unsigned)p;
  }
  return w;
}

// One lane group (D / 16 lanes) per (b, t, head row of q | k | v). Groups are whole: the thread count and the
// block size are multiples of D / 16, and every branch below is taken by all the lanes of a group.
// RING: the rotation takes the absolute position lens[b] + t, the store goes to slot (lens[b] + t) % Tcap and no row is
// dropped. The host refuses a step without a table row for every position; a device-side lens beyond what the host
// believed is still kept inside the table here: such a row is neither rotated nor stored.
// PAGED: position p = lens[b] + t goes to page pt[b][p >> 8], row p & 255; a position at or beyond Tcap, or whose
// table entry lies outside [0, n_pages), or without a table row (p >= max_pos), is neither rotated nor stored (uniform
// over a head row's lanes).
template <int D, bool F8, bool RING, bool PAGED>
__global__ __launch_bounds__(256) void kv_append_rope(
    std::conditional_t<PAGED, PagedAppendArgs, std::conditional_t<RING, RingAppendArgs, AppendArgs>> a) {
  static_assert(!PAGED || !RING, "a paged cache is no ring");
  constexpr int G = D / 16;
  const int NH = a.Hq + 2 * a.Hkv;
  const long long n = (long long)a.B * a.T * NH * G;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int j = (int)(r % G);
  r /= G;
  const int hh = (int)(r % NH);
  r /= NH;
  const int t = (int)(r % a.T);
  const int b = (int)(r / a.T);
  const long long row = (long long)a.lens[b] + t;
  long long slot = row;  // the cache row
  if constexpr (RING) {
    if (row < 0 || row >= a.max_pos) return;
    slot = (unsigned)row % (unsigned)a.Tcap;
  } else {
    if (row < 0 || row >= a.Tcap) return;  // past the capacity: neither appended nor rotated
  }
  long long sl = b;  // the slice of the cache's first dimension
  if constexpr (PAGED) {
    if (row >= a.max_pos) return;
    sl = a.pt[b * a.pts + (row >> 8)];
    if (sl < 0 || sl >= a.n_pages) return;  // no page: dropped
    slot = row & 255;
  }
  __bf16* src = a.qkv + b * a.qb + t * a.qt + (long long)hh * D + j * 8;
  u32x4 lo = *reinterpret_cast<const u32x4*>(src);
  u32x4 hi = *reinterpret_cast<const u32x4*>(src + D / 2);
  const bool is_v = hh >= a.Hq + a.Hkv;
  if (!is_v) {  // q and k: rotated in place
    rotate16<D>(lo, hi, a.table + row * D + j * 8, 1.f);
    *reinterpret_cast<u32x4*>(src) = lo;
    *reinterpret_cast<u32x4*>(src + D / 2) = hi;
    if (hh < a.Hq) return;
  }
  const int h = is_v ? hh - a.Hq - a.Hkv : hh - a.Hq;
  if constexpr (!F8) {
    __bf16* dst = is_v ? static_cast<__bf16*>(a.vc) + sl * a.vb + h * a.vh + slot * a.vt
                       : static_cast<__bf16*>(a.kc) + sl * a.kb + h * a.kh + slot * a.kt;
    *reinterpret_cast<u32x4*>(dst + j * 8) = lo;
    *reinterpret_cast<u32x4*>(dst + D / 2 + j * 8) = hi;
  } else {
    float x[16];
    Bf16Rows::unpack8(lo, x);
    Bf16Rows::unpack8(hi, x + 8);
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) am = fmaxf(am, fabsf(x[i]));
    am = kfw::group_max<G>(am);
    const float scale = am > 0.f ? am / kFp8Max : 1.f;  // IEEE division: the torch reference's scale
    uint8_t* dst = is_v ? static_cast<uint8_t*>(a.vc) + sl * a.vb + h * a.vh + slot * a.vt
                        : static_cast<uint8_t*>(a.kc) + sl * a.kb + h * a.kh + slot * a.kt;
    *reinterpret_cast<u32x2*>(dst + j * 8) = fp8_codes(x, scale);
    *reinterpret_cast<u32x2*>(dst + D / 2 + j * 8) = fp8_codes(x + 8, scale);
    if (j == 0) {
      float* sd = is_v ? a.vs + sl * a.vsb + h * a.vsh : a.ks + sl * a.ksb + h * a.ksh;
      sd[slot] = scale;
    }
  }
}

template <bool F8, bool RING = false, bool PAGED = false>
int append_rope(void* qkv, void* kc, void* vc, float* ks, float* vs, const int* lens, const float* table, int max_pos,
                int B, int T, int Hq, int Hkv, int D, int Tcap, long long qb, long long qt, const long long* c,
                void* stream, const int* pt = nullptr, long long pts = 0, int n_pages = 0) {
  if (PAGED && (!pt || n_pages < 1 || Tcap <= 0 || Tcap % kSplitKeys || pts < Tcap / kSplitKeys || !al4(pt)))
    return KFAMD_EINVAL;
  if (!qkv || !kc || !vc || !lens || !table || !c || B <= 0 || T <= 0 || Hkv <= 0 || Tcap <= 0 || Hq < Hkv ||
      Hq % Hkv || group_log2(Hq / Hkv) < 0)
    return KFAMD_EINVAL;
  if (F8 && (!ks || !vs)) return KFAMD_EINVAL;
  if (D != 64 && D != 128) return KFAMD_EINVAL;
  if (RING ? (max_pos < 1 || Tcap % kSplitKeys || T > Tcap) : PAGED ? max_pos < 1 : max_pos < Tcap) return KFAMD_EINVAL;  // flat: every cache row has a table row
  if (c[2] < D || c[5] < D) return KFAMD_EINVAL;
  if (!al16(qkv) || !al16(kc) || !al16(vc) || !al16(table)) return KFAMD_EALIGN;
  if (F8 && (!al4(ks) || !al4(vs))) return KFAMD_EALIGN;
  if ((qb | qt) & 7) return KFAMD_EALIGN;
  if ((c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & (F8 ? 15 : 7)) return KFAMD_EALIGN;
  const long long n = (long long)B * T * (Hq + 2 * Hkv) * (D / 16);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  std::conditional_t<PAGED, PagedAppendArgs, std::conditional_t<RING, RingAppendArgs, AppendArgs>> a = {};
  if constexpr (RING) a.max_pos = max_pos;
  if constexpr (PAGED) a.pt = pt, a.pts = pts, a.n_pages = n_pages, a.max_pos = max_pos;
  a.qkv = static_cast<__bf16*>(qkv);
  a.kc = kc, a.vc = vc, a.ks = ks, a.vs = vs, a.lens = lens, a.table = table;
  a.B = B, a.T = T, a.Hq = Hq, a.Hkv = Hkv, a.Tcap = Tcap;
  a.qb = qb, a.qt = qt, a.kb = c[0], a.kh = c[1], a.kt = c[2], a.vb = c[3], a.vh = c[4], a.vt = c[5];
  if (F8) a.ksb = c[6], a.ksh = c[7], a.vsb = c[8], a.vsh = c[9];
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (D == 64) hipLaunchKernelGGL((kv_append_rope<64, F8, RING, PAGED>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((kv_append_rope<128, F8, RING, PAGED>), grid, dim3(256), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

extern "C" int kfamd_rope_qkv_bf16(void* qkv, const float* table, const int* pos, int max_pos, int B, int T, int Hq,
                                   int Hkv, int D, long long qb, long long qt, int inverse, void* stream) {
  if (!qkv || !table || B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || max_pos <= 0) return KFAMD_EINVAL;
  if (D != 64 && D != 128) return KFAMD_EINVAL;
  if (!al16(qkv) || !al16(table)) return KFAMD_EALIGN;
  if ((qb | qt) & 7) return KFAMD_EALIGN;
  const int NH = Hq + Hkv;
  const long long n = (long long)B * T * NH * (D / 16);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  __bf16* x = static_cast<__bf16*>(qkv);
  const float sign = inverse ? -1.f : 1.f;
  if (D == 64) hipLaunchKernelGGL(rope_qkv<64>, grid, dim3(256), 0, s, x, table, pos, B, T, NH, max_pos, qb, qt, sign);
  else hipLaunchKernelGGL(rope_qkv<128>, grid, dim3(256), 0, s, x, table, pos, B, T, NH, max_pos, qb, qt, sign);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

extern "C" int kfamd_kv_append_rope_bf16(void* qkv, void* k_cache, void* v_cache, const int* lens, const float* table,
                                         int max_pos, int B, int T, int Hq, int Hkv, int D, int Tcap, long long qb,
                                         long long qt, const long long* cache_strides, void* stream) {
  return append_rope<false>(qkv, k_cache, v_cache, nullptr, nullptr, lens, table, max_pos, B, T, Hq, Hkv, D, Tcap, qb,
                            qt, cache_strides, stream);
}

extern "C" int kfamd_kv_append_rope_fp8(void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                        const int* lens, const float* table, int max_pos, int B, int T, int Hq, int Hkv,
                                        int D, int Tcap, long long qb, long long qt, const long long* cache_strides,
                                        void* stream) {
  return append_rope<true>(qkv, k_codes, v_codes, k_scale, v_scale, lens, table, max_pos, B, T, Hq, Hkv, D, Tcap, qb, qt,
                           cache_strides, stream);
}

// The ring forms: positions lens[b] + t are absolute (the table needs a row for each: max_pos >= the largest
// lens[b] + T, which the caller checks; a position at or beyond max_pos is neither rotated nor stored), the store goes to slot
// (lens[b] + t) % cap; cap a multiple of 256, T <= cap.
extern "C" int kfamd_kv_append_rope_ring_bf16(void* qkv, void* k_cache, void* v_cache, const int* lens,
                                              const float* table, int max_pos, int B, int T, int Hq, int Hkv, int D,
                                              int cap, long long qb, long long qt, const long long* cache_strides,
                                              void* stream) {
  return append_rope<false, true>(qkv, k_cache, v_cache, nullptr, nullptr, lens, table, max_pos, B, T, Hq, Hkv, D, cap,
                                  qb, qt, cache_strides, stream);
}

extern "C" int kfamd_kv_append_rope_ring_fp8(void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                             const int* lens, const float* table, int max_pos, int B, int T, int Hq,
                                             int Hkv, int D, int cap, long long qb, long long qt,
                                             const long long* cache_strides, void* stream) {
  return append_rope<true, true>(qkv, k_codes, v_codes, k_scale, v_scale, lens, table, max_pos, B, T, Hq, Hkv, D, cap,
                                 qb, qt, cache_strides, stream);
}

// The paged forms (the page rule: ops/decode.py): kfamd_kv_append_rope_bf16 / _fp8 with the page table before the
// stream; cap is the row capacity (a multiple of 256), the b entries of cache_strides are the page strides. The table
// need not reach cap (max_pos >= 1): a position at or beyond max_pos is neither rotated nor stored, the caller checks.
extern "C" int kfamd_kv_append_rope_paged_bf16(void* qkv, void* k_pages, void* v_pages, const int* lens,
                                               const float* table, int max_pos, int B, int T, int Hq, int Hkv, int D,
                                               int cap, long long qb, long long qt, const long long* cache_strides,
                                               const int* page_table, long long table_stride, int n_pages,
                                               void* stream) {
  return append_rope<false, false, true>(qkv, k_pages, v_pages, nullptr, nullptr, lens, table, max_pos, B, T, Hq, Hkv,
                                         D, cap, qb, qt, cache_strides, stream, page_table, table_stride, n_pages);
}

extern "C" int kfamd_kv_append_rope_paged_fp8(void* qkv, void* k_pages, void* v_pages, float* k_scale, float* v_scale,
                                              const int* lens, const float* table, int max_pos, int B, int T, int Hq,
                                              int Hkv, int D, int cap, long long qb, long long qt,
                                              const long long* cache_strides, const int* page_table,
                                              long long table_stride, int n_pages, void* stream) {
  return append_rope<true, false, true>(qkv, k_pages, v_pages, k_scale, v_scale, lens, table, max_pos, B, T, Hq, Hkv, D,
                                        cap, qb, qt, cache_strides, stream, page_table, table_stride, n_pages);
}
