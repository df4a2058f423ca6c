// attn_kv_fp8.hip — the FP8 KV cache: quantising append, single-query and multi-query attention.
//
// The cache holds OCP e4m3fn codes [B][H][Tcap][D] (one byte per element) and one fp32 scale per stored
// row ([B][H][Tcap], one tensor for K and one for V). A row x[0..D) of bf16 values read as fp32 is stored
// as
//     scale = max|x| / 448   (1 for an all-zero row),   code = RNE_e4m3(clamp(x / scale, -448, 448)),
// clamped in fp32 before v_cvt_pk_fp8_f32 so that nothing depends on the hardware's FP8 overflow mode;
// code * scale gives the row back. Neither attention kernel dequantises to memory: the codes are
// unpacked to fp32 on the VALU (v_cvt_pk_f32_fp8, 4 per 8 elements where bf16 takes 8 shifts / ands),
// the score of key j is (q . codes_k[j]) * kscale[j], and vscale[j] is folded into p before the P.V
// FMAs. Everything else — the split structure, the per-row causal limit, the empty-split handling, the
// fp32 workspace and the combine launches — is attn_decode_bf16.hip's and attn_extend_bf16.hip's; the
// combines read only the workspace and are shared (kfamd_attn_decode_combine / _extend_combine).
//
// Load width: a key row is D BYTES here, and a lane takes 8 of them in one 8-B load, so a row is still
// D / 8 lanes wide. The 16-B form (D / 16 lanes) was not built: at D = 64 it leaves 4-lane groups, which
// wave_ops.h's group reductions do not cover, and it doubles the accumulators per lane (16 dims per row
// slot), which at R = 8 row slots is 128 VGPRs of accumulators alone next to 128 of q: a certain spill.
// With 8 B per lane the lane groups, the keys per block step and the accumulators per lane are the bf16
// kernels', and the static_assert that a split holds a whole number of block steps holds as it stands.
// A wave still reads 512 contiguous bytes per load instruction (dense rows), half of bf16's; kUnroll
// keys per lane group and step are loaded ahead to keep bytes in flight. The scale of key j is loaded
// with its row (every lane of the group reads the same word) and prefetched with it.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch is 0
// for every instantiation):
//   kernel                                   VGPRs (D = 64 / 128)   scratch
//   kv_append_fp8<D>                          39 /  39               0
//   attn_decode_split_fp8<D>                  84 /  84               0
//   attn_extend_split_fp8<D, 1>               97 /  84               0
//   attn_extend_split_fp8<D, 2>              116 / 116               0
//   attn_extend_split_fp8<D, 4>              150 / 150               0
//   attn_extend_split_fp8<D, 8>              198 / 198               0   (bf16: 202)
// Measured against the bf16 kernels (profiles/kv_fp8, D = 128, capacity 4096): decode 1.57-1.71x faster
// at B*H = 128 with 2048 / 4096 keys; extend at Tq = 4 1.17x at 2048 keys and a tie at 4096, where the
// per-row VALU work (the same FMAs as bf16) sets the time; extend at Tq = 8 ties or loses 4 %; ties within
// the launch floor at 128 keys and at B*H = 16. The append is 1.33x slower at T = 2048 (8 IEEE divisions
// per lane): 63 us per layer of a 2048-token prefill.
//
// Keys at or beyond a row's limit are excluded by a branch on the key index, never multiplied by
// zero: codes there may be 0x7F (NaN) and scales NaN. Addresses, the scale loads' too, are clamped to
// a valid key. lens is DEVICE memory and is never advanced here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kSplitKeys = 256;  // must equal kfamd_attn_decode_split_keys(): checked by the launchers
constexpr int kThreads = 256;
// keys per lane group and block step, loaded one step ahead. A lane's load is 8 B here, half of bf16's:
// twice bf16's unroll keeps the same bytes in flight where the kernel is a KV stream (decode, extend
// up to 4 row slots); at 8 row slots the VALU sets the time and the registers go to the accumulators.
constexpr int kUnrollStream = 4;
constexpr int kUnrollRows8 = 2;
constexpr int kMaxRows = 16;
constexpr int kSlotRows = 8;   // query rows per split launch
constexpr int kMergeRows = 4;  // row slots merged per LDS pass
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kFp8Max = 448.f;  // largest finite e4m3fn value (code 0x7E)

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ void unpack8_bf16(const u32x4& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf_lo(w[i]);
    f[2 * i + 1] = bf_hi(w[i]);
  }
}

// 8 e4m3 codes (memory order: byte 0 first) -> fp32
__device__ __forceinline__ void unpack8_fp8(const u32x2& w, float* f) {
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

// ---- append ------------------------------------------------------------------------------------
// One lane group (D / 8 lanes) per (b, t, k-or-v, h) row: a 16-B load of 8 bf16 per lane, the row's
// amax by the group reduction, one scale store by the group's first lane, one 8-B code store per lane.
// Groups are whole: the thread count is a multiple of D / 8 and so is the block size, and both early
// returns are group-uniform.
template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8(const __bf16* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                     uint8_t* __restrict__ vc, float* __restrict__ ks,
                                                     float* __restrict__ vs, const int* __restrict__ pos, int B, int T,
                                                     int H, int Tcap, long long qb, long long qt, long long kb,
                                                     long long kh, long long kt, long long vb, long long vh,
                                                     long long vt, long long ksb, long long ksh, long long vsb,
                                                     long long vsh) {
  constexpr int G = D / 8;
  const long long n = (long long)B * T * 2 * H * G;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int piece = (int)(r % G);
  r /= G;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % 2);  // 0: k, 1: v
  r /= 2;
  const int t = (int)(r % T);
  const int b = (int)(r / T);
  const long long row = (long long)pos[b] + t;
  if (row < 0 || row >= Tcap) return;  // past the capacity: dropped, neither codes nor scale written
  float x[8];
  unpack8_bf16(*reinterpret_cast<const u32x4*>(qkv + b * qb + t * qt + ((long long)(s + 1) * H + h) * D + piece * 8),
               x);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
  am = kfw::group_max<G>(am);
  const float scale = am > 0.f ? am / kFp8Max : 1.f;  // IEEE division: the torch reference's scale
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
  uint8_t* dst = s == 0 ? kc + b * kb + h * kh + row * kt : vc + b * vb + h * vh + row * vt;
  *reinterpret_cast<u32x2*>(dst + piece * 8) = w;
  if (piece == 0) {
    float* sd = s == 0 ? ks + b * ksb + h * ksh : vs + b * vsb + h * vsh;
    sd[row] = scale;
  }
}

// ---- decode ------------------------------------------------------------------------------------
struct DecodeArgs {
  const __bf16* q;
  const uint8_t* k;
  const uint8_t* v;
  const float* ks;
  const float* vs;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int H, t_bound, nsplit;
  float scale_log2;
  long long qb, qh, kb, kh, kt, vb, vh, vt, ob, oh, ksb, ksh, vsb, vsh;
};

// workspace: [B][H][nsplit][2] (m, l) then [B][H][nsplit][D] (o), fp32 — attn_decode_bf16.hip's
template <int D>
__global__ __launch_bounds__(kThreads) void attn_decode_split_fp8(DecodeArgs a) {
  constexpr int kUnroll = kUnrollStream;
  constexpr int G = D / 8;             // lanes per key row (8 B per lane)
  constexpr int NG = kThreads / G;     // lane groups per block (= keys per block and unroll slot)
  constexpr int KSTEP = NG * kUnroll;  // keys per block step
  static_assert(kSplitKeys % KSTEP == 0, "a split holds a whole number of block steps");
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int grp = tid / G, piece = tid % G;

  __shared__ float s_m[NG], s_l[NG];
  __shared__ float s_o[NG][D + 4];

  int len = a.lens[b];
  len = len < 0 ? 0 : (len > a.t_bound ? a.t_bound : len);
  const int k0 = split * kSplitKeys;
  const int k1 = min(k0 + kSplitKeys, len);  // valid keys of this split: [k0, k1)
  const long long bh = ((long long)b * a.H + h);
  float* ws_ml = a.ws + (bh * a.nsplit + split) * 2;
  float* ws_o = a.ws + (long long)gridDim.z * a.H * a.nsplit * 2 + (bh * a.nsplit + split) * D;

  if (k1 <= k0) {  // empty split (only reachable with nsplit > 1 or len == 0)
    if (a.nsplit > 1) {
      if (tid == 0) {
        ws_ml[0] = -INFINITY;
        ws_ml[1] = 0.f;
      }
      if (tid < D) ws_o[tid] = 0.f;
    } else {
      if (tid < D) a.o[b * a.ob + h * a.oh + tid] = (__bf16)0.f;
      if (tid == 0 && a.lse) a.lse[bh] = -INFINITY;
    }
    return;
  }

  float qf[8];
  unpack8_bf16(*reinterpret_cast<const u32x4*>(a.q + b * a.qb + h * a.qh + piece * 8), qf);
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[i] *= a.scale_log2;

  const uint8_t* kbase = a.k + b * a.kb + h * a.kh + piece * 8;
  const uint8_t* vbase = a.v + b * a.vb + h * a.vh + piece * 8;
  const float* ksbase = a.ks + b * a.ksb + h * a.ksh;
  const float* vsbase = a.vs + b * a.vsb + h * a.vsh;
  const int last = k1 - 1;  // addresses are clamped to a valid key; the key index decides validity

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  u32x2 kn[kUnroll], vn[kUnroll];
  float ksn[kUnroll], vsn[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int key = min(k0 + u * NG + grp, last);
    kn[u] = *reinterpret_cast<const u32x2*>(kbase + key * a.kt);
    vn[u] = *reinterpret_cast<const u32x2*>(vbase + key * a.vt);
    ksn[u] = ksbase[key];
    vsn[u] = vsbase[key];
  }
  for (int kk = k0; kk < k1; kk += KSTEP) {
    u32x2 kc[kUnroll], vc[kUnroll];
    float ksc[kUnroll], vsc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      kc[u] = kn[u];
      vc[u] = vn[u];
      ksc[u] = ksn[u];
      vsc[u] = vsn[u];
    }
    if (kk + KSTEP < k1) {  // the next step's loads go out before this step's arithmetic
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int key = min(kk + KSTEP + u * NG + grp, last);
        kn[u] = *reinterpret_cast<const u32x2*>(kbase + key * a.kt);
        vn[u] = *reinterpret_cast<const u32x2*>(vbase + key * a.vt);
        ksn[u] = ksbase[key];
        vsn[u] = vsbase[key];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int key = kk + u * NG + grp;
      float kf[8];
      unpack8_fp8(kc[u], kf);
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) part = fmaf(qf[i], kf[i], part);
      const float s = kfw::group_sum<G>(part) * ksc[u];  // scale * log2e * q.(codes * kscale)
      if (key < k1) {                                    // group-uniform; an invalid key touches no state
        float vf[8];
        unpack8_fp8(vc[u], vf);
        const float mn = fmaxf(m, s);
        const float corr = exp2f(m - mn);  // m = -inf on the first key: exp2(-inf) = 0
        const float p = exp2f(s - mn);
        l = l * corr + p;
        const float pv = p * vsc[u];  // V's scale folded into p
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(acc[i], corr, pv * vf[i]);
        m = mn;
      }
    }
  }

  // the block's lane groups meet in LDS
  if (piece == 0) {
    s_m[grp] = m;
    s_l[grp] = l;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) s_o[grp][piece * 8 + i] = acc[i];
  __syncthreads();
  if (tid < D) {
    float M = -INFINITY;
    for (int g = 0; g < NG; ++g) M = fmaxf(M, s_m[g]);  // finite: the split holds at least one key
    float L = 0.f, O = 0.f;
    for (int g = 0; g < NG; ++g) {
      const float mg = s_m[g];
      const float w = mg == -INFINITY ? 0.f : exp2f(mg - M);  // a group that saw no key
      L += s_l[g] * w;
      O += s_o[g][tid] * w;
    }
    if (a.nsplit > 1) {
      ws_o[tid] = O;
      if (tid == 0) {
        ws_ml[0] = M;
        ws_ml[1] = L;
      }
    } else {
      a.o[b * a.ob + h * a.oh + tid] = (__bf16)(O / L);
      if (tid == 0 && a.lse) a.lse[bh] = (M + log2f(L)) * kLn2;
    }
  }
}

// ---- extend ------------------------------------------------------------------------------------
struct ExtendArgs {
  const __bf16* q;
  const uint8_t* k;
  const uint8_t* v;
  const float* ks;
  const float* vs;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int H, Tq, row0, t_bound, nsplit;  // this launch holds rows row0 .. row0 + R - 1 of the Tq
  float scale_log2;
  long long qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh, ksb, ksh, vsb, vsh;
};

// workspace: [B][H][Tq][nsplit][2] (m, l) then [B][H][Tq][nsplit][D] (o), fp32 — attn_extend_bf16.hip's
template <int D, int R>
__global__ __launch_bounds__(kThreads) void attn_extend_split_fp8(ExtendArgs a) {
  constexpr int kUnroll = R >= 8 ? kUnrollRows8 : kUnrollStream;
  constexpr int G = D / 8;             // lanes per key row (8 B per lane)
  constexpr int NG = kThreads / G;     // lane groups per block
  constexpr int KSTEP = NG * kUnroll;  // keys per block step
  constexpr int RC = R < kMergeRows ? R : kMergeRows;
  // a block step never reaches into the next split: `key < nk[r]` alone then decides a key's validity
  static_assert(kSplitKeys % KSTEP == 0, "a split holds a whole number of block steps");
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int grp = tid / G, piece = tid % G;
  const int Tq = a.Tq;

  __shared__ float s_m[NG][RC], s_l[NG][RC];
  __shared__ float s_o[NG][RC][D + 4];

  int len = a.lens[b];
  len = len < 0 ? 0 : (len > a.t_bound ? a.t_bound : len);
  const int k0 = split * kSplitKeys;
  const int k1 = min(k0 + kSplitKeys, len);  // keys of this split that the last row may see: [k0, k1)
  const long long bh = (long long)b * a.H + h;
  const long long nrows = (long long)gridDim.z * a.H * Tq;  // B * H * Tq

  if (k1 <= k0) {  // empty split for every row (block-uniform, before any barrier)
    for (int r = a.row0; r < min(a.row0 + R, Tq); ++r) {
      const long long row = bh * Tq + r;
      if (a.nsplit > 1) {
        if (tid == 0) {
          a.ws[(row * a.nsplit + split) * 2] = -INFINITY;
          a.ws[(row * a.nsplit + split) * 2 + 1] = 0.f;
        }
        if (tid < D) a.ws[nrows * a.nsplit * 2 + (row * a.nsplit + split) * D + tid] = 0.f;
      } else {
        if (tid < D) a.o[b * a.ob + r * a.ot + h * a.oh + tid] = (__bf16)0.f;
        if (tid == 0 && a.lse) a.lse[((long long)b * Tq + r) * a.H + h] = -INFINITY;
      }
    }
    return;
  }

  // row slot r sees keys [0, nk[r]); a padding slot (r >= Tq) and a row before the sequence's start see none
  float qf[R][8];
  int nk[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gr = a.row0 + r;             // the slot's row of the Tq
    const int rr = gr < Tq ? gr : Tq - 1;  // padding slots read a valid row
    unpack8_bf16(*reinterpret_cast<const u32x4*>(a.q + b * a.qb + rr * a.qt + h * a.qh + piece * 8), qf[r]);
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[r][i] *= a.scale_log2;
    nk[r] = gr < Tq ? len - Tq + gr + 1 : 0;
  }

  const uint8_t* kbase = a.k + b * a.kb + h * a.kh + piece * 8;
  const uint8_t* vbase = a.v + b * a.vb + h * a.vh + piece * 8;
  const float* ksbase = a.ks + b * a.ksb + h * a.ksh;
  const float* vsbase = a.vs + b * a.vsb + h * a.vsh;
  const int last = k1 - 1;  // addresses are clamped to a valid key; the key index decides validity

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }

  u32x2 kn[kUnroll], vn[kUnroll];
  float ksn[kUnroll], vsn[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int key = min(k0 + u * NG + grp, last);
    kn[u] = *reinterpret_cast<const u32x2*>(kbase + key * a.kt);
    vn[u] = *reinterpret_cast<const u32x2*>(vbase + key * a.vt);
    ksn[u] = ksbase[key];
    vsn[u] = vsbase[key];
  }
  for (int kk = k0; kk < k1; kk += KSTEP) {
    u32x2 kc[kUnroll], vc[kUnroll];
    float ksc[kUnroll], vsc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      kc[u] = kn[u];
      vc[u] = vn[u];
      ksc[u] = ksn[u];
      vsc[u] = vsn[u];
    }
    if (kk + KSTEP < k1) {  // the next step's loads go out before this step's arithmetic
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int key = min(kk + KSTEP + u * NG + grp, last);
        kn[u] = *reinterpret_cast<const u32x2*>(kbase + key * a.kt);
        vn[u] = *reinterpret_cast<const u32x2*>(vbase + key * a.vt);
        ksn[u] = ksbase[key];
        vsn[u] = vsbase[key];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int key = kk + u * NG + grp;
      float kf[8], vf[8];
      unpack8_fp8(kc[u], kf);
      unpack8_fp8(vc[u], vf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) part = fmaf(qf[r][i], kf[i], part);
        const float s = kfw::group_sum<G>(part) * ksc[u];  // scale * log2e * q_r.(codes * kscale)
        if (key < nk[r]) {                                 // group-uniform; an invalid key touches no state
          const float mn = fmaxf(m[r], s);
          const float corr = exp2f(m[r] - mn);  // m = -inf on the first key: exp2(-inf) = 0
          const float p = exp2f(s - mn);
          l[r] = l[r] * corr + p;
          const float pv = p * vsc[u];  // V's scale folded into p
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(acc[r][i], corr, pv * vf[i]);
          m[r] = mn;
        }
      }
    }
  }

  // the block's lane groups meet in LDS, RC row slots per pass
#pragma unroll
  for (int r0 = 0; r0 < R; r0 += RC) {
    if (a.row0 + r0 >= Tq) break;  // block-uniform: only padding slots are left
    if (r0 > 0) __syncthreads();   // the previous pass has been read
#pragma unroll
    for (int j = 0; j < RC; ++j) {
      if (piece == 0) {
        s_m[grp][j] = m[r0 + j];
        s_l[grp][j] = l[r0 + j];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s_o[grp][j][piece * 8 + i] = acc[r0 + j][i];
    }
    __syncthreads();
    for (int item = tid; item < RC * D; item += kThreads) {
      const int j = item / D, d = item % D;
      const int r = a.row0 + r0 + j;
      if (r >= Tq) continue;  // padding: nothing of it is stored
      float M = -INFINITY;
      for (int g = 0; g < NG; ++g) M = fmaxf(M, s_m[g][j]);
      float L = 0.f, O = 0.f;
      for (int g = 0; g < NG; ++g) {
        const float mg = s_m[g][j];
        const float w = mg == -INFINITY ? 0.f : exp2f(mg - M);  // a group that saw no key of this row
        L += s_l[g][j] * w;
        O += s_o[g][j][d] * w;
      }
      const long long row = bh * Tq + r;
      if (a.nsplit > 1) {  // M = -inf, L = 0 for a row with no key in this split
        a.ws[nrows * a.nsplit * 2 + (row * a.nsplit + split) * D + d] = O;
        if (d == 0) *reinterpret_cast<float2*>(a.ws + (row * a.nsplit + split) * 2) = make_float2(M, L);
      } else {
        const bool any = L > 0.f;  // a row before the sequence's start (lens[b] < Tq) sees no key
        a.o[b * a.ob + r * a.ot + h * a.oh + d] = (__bf16)(any ? O / L : 0.f);
        if (d == 0 && a.lse) a.lse[((long long)b * Tq + r) * a.H + h] = any ? (M + log2f(L)) * kLn2 : -INFINITY;
      }
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int D>
void launch_extend(int R, dim3 grid, hipStream_t s, const ExtendArgs& a) {
  switch (R) {
    case 1: hipLaunchKernelGGL((attn_extend_split_fp8<D, 1>), grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL((attn_extend_split_fp8<D, 2>), grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL((attn_extend_split_fp8<D, 4>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((attn_extend_split_fp8<D, 8>), grid, dim3(kThreads), 0, s, a); break;
  }
}

// the checks the two attention launchers share: code strides are bytes, multiples of 16; q / o strides
// are bf16 elements, multiples of 8; a (b, h) slice of codes stays below 2^31 bytes
int check_cache(const void* k, const void* v, const float* ks, const float* vs, int D, int t_bound, long long kt,
                long long vt) {
  if (!k || !v || !ks || !vs) return KFAMD_EINVAL;
  if ((D != 64 && D != 128) || t_bound < 1) return KFAMD_EINVAL;
  if (kfamd_attn_decode_split_keys() != kSplitKeys) return KFAMD_EINVAL;
  if (kt < D || vt < D) return KFAMD_EINVAL;
  const long long lim = 1ll << 31;
  if ((long long)t_bound * kt >= lim || (long long)t_bound * vt >= lim) return KFAMD_EINVAL;
  if (!al16(k) || !al16(v) || (reinterpret_cast<uintptr_t>(ks) & 3) || (reinterpret_cast<uintptr_t>(vs) & 3))
    return KFAMD_EALIGN;
  return KFAMD_OK;
}

}  // namespace

// K and V rows of a fused QKV activation [B][T][3][H][D] (element strides qb, qt; [3][H][D] dense),
// quantised row by row into codes [B][H][Tcap][D] and scales [B][H][Tcap] at rows pos[b] .. pos[b] + T - 1.
// cache_strides = {kb, kh, kt, vb, vh, vt, ksb, ksh, vsb, vsh}.
extern "C" int kfamd_kv_append_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                   const int* pos, int B, int T, int H, int D, int Tcap, long long qb, long long qt,
                                   const long long* cache_strides, void* stream) {
  if (!qkv || !k_codes || !v_codes || !k_scale || !v_scale || !pos || !cache_strides || B <= 0 || T <= 0 || H <= 0 ||
      Tcap <= 0)
    return KFAMD_EINVAL;
  if (D != 64 && D != 128) return KFAMD_EINVAL;
  const long long* c = cache_strides;
  if (c[2] < D || c[5] < D) return KFAMD_EINVAL;
  if (!al16(qkv) || !al16(k_codes) || !al16(v_codes) || (reinterpret_cast<uintptr_t>(k_scale) & 3) ||
      (reinterpret_cast<uintptr_t>(v_scale) & 3))
    return KFAMD_EALIGN;
  if ((qb | qt) & 7) return KFAMD_EALIGN;
  if ((c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & 15) return KFAMD_EALIGN;
  const long long n = (long long)B * T * 2 * H * (D / 8);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const __bf16* x = static_cast<const __bf16*>(qkv);
  uint8_t* kc = static_cast<uint8_t*>(k_codes);
  uint8_t* vc = static_cast<uint8_t*>(v_codes);
  if (D == 64)
    hipLaunchKernelGGL(kv_append_fp8<64>, grid, dim3(256), 0, s, x, kc, vc, k_scale, v_scale, pos, B, T, H, Tcap, qb, qt,
                       c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]);
  else
    hipLaunchKernelGGL(kv_append_fp8<128>, grid, dim3(256), 0, s, x, kc, vc, k_scale, v_scale, pos, B, T, H, Tcap, qb,
                       qt, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

// strides: q (b, h), k_codes (b, h, t), v_codes (b, h, t), o (b, h), k_scale (b, h), v_scale (b, h) — 14 values
extern "C" int kfamd_attn_decode_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                     const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                     int D, int t_bound, float scale, const long long* st, void* stream) {
  if (!q || !lens || !o || !st || B <= 0 || H <= 0 || B > 65535 || H > 65535) return KFAMD_EINVAL;
  const long long qb = st[0], qh = st[1], kb = st[2], kh = st[3], kt = st[4], vb = st[5], vh = st[6], vt = st[7],
                  ob = st[8], oh = st[9];
  const int rc = check_cache(k_codes, v_codes, k_scale, v_scale, D, t_bound, kt, vt);
  if (rc == KFAMD_EINVAL) return rc;
  const int nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  if (nsplit > 1 && !ws) return KFAMD_EINVAL;
  if (rc != KFAMD_OK) return rc;
  if (!al16(q) || !al16(o) || (ws && !al16(ws))) return KFAMD_EALIGN;
  if ((qb | qh | ob | oh) & 7) return KFAMD_EALIGN;
  if ((kb | kh | kt | vb | vh | vt) & 15) return KFAMD_EALIGN;
  DecodeArgs a;
  a.q = static_cast<const __bf16*>(q);
  a.k = static_cast<const uint8_t*>(k_codes);
  a.v = static_cast<const uint8_t*>(v_codes);
  a.ks = k_scale;
  a.vs = v_scale;
  a.lens = lens;
  a.o = static_cast<__bf16*>(o);
  a.lse = lse;
  a.ws = static_cast<float*>(ws);
  a.H = H;
  a.t_bound = t_bound;
  a.nsplit = nsplit;
  a.scale_log2 = scale * kLog2e;
  a.qb = qb, a.qh = qh, a.kb = kb, a.kh = kh, a.kt = kt, a.vb = vb, a.vh = vh, a.vt = vt, a.ob = ob, a.oh = oh;
  a.ksb = st[10], a.ksh = st[11], a.vsb = st[12], a.vsh = st[13];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nsplit, (unsigned)H, (unsigned)B);
  if (D == 64) hipLaunchKernelGGL(attn_decode_split_fp8<64>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(attn_decode_split_fp8<128>, grid, dim3(kThreads), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (nsplit > 1) return kfamd_attn_decode_combine(a.ws, a.o, lse, B, H, D, nsplit, ob, oh, stream);
  return KFAMD_OK;
}

// strides: q (b, t, h), k_codes (b, h, t), v_codes (b, h, t), o (b, t, h), k_scale (b, h), v_scale (b, h) — 16 values
extern "C" int kfamd_attn_extend_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                     const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                     int D, int Tq, int t_bound, float scale, const long long* st, void* stream) {
  if (!q || !lens || !o || !st || B <= 0 || H <= 0 || B > 65535 || H > 65535) return KFAMD_EINVAL;
  if (Tq < 1 || Tq > kMaxRows) return KFAMD_EINVAL;
  const long long qb = st[0], qt = st[1], qh = st[2], kb = st[3], kh = st[4], kt = st[5], vb = st[6], vh = st[7],
                  vt = st[8], ob = st[9], ot = st[10], oh = st[11];
  const int rc = check_cache(k_codes, v_codes, k_scale, v_scale, D, t_bound, kt, vt);
  if (rc == KFAMD_EINVAL) return rc;
  const int nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  if (nsplit > 1 && !ws) return KFAMD_EINVAL;
  if (rc != KFAMD_OK) return rc;
  if (!al16(q) || !al16(o) || (ws && !al16(ws))) return KFAMD_EALIGN;
  if ((qb | qt | qh | ob | ot | oh) & 7) return KFAMD_EALIGN;
  if ((kb | kh | kt | vb | vh | vt) & 15) return KFAMD_EALIGN;
  ExtendArgs a;
  a.q = static_cast<const __bf16*>(q);
  a.k = static_cast<const uint8_t*>(k_codes);
  a.v = static_cast<const uint8_t*>(v_codes);
  a.ks = k_scale;
  a.vs = v_scale;
  a.lens = lens;
  a.o = static_cast<__bf16*>(o);
  a.lse = lse;
  a.ws = static_cast<float*>(ws);
  a.H = H;
  a.Tq = Tq;
  a.t_bound = t_bound;
  a.nsplit = nsplit;
  a.scale_log2 = scale * kLog2e;
  a.qb = qb, a.qt = qt, a.qh = qh, a.kb = kb, a.kh = kh, a.kt = kt, a.vb = vb, a.vh = vh, a.vt = vt;
  a.ob = ob, a.ot = ot, a.oh = oh;
  a.ksb = st[12], a.ksh = st[13], a.vsb = st[14], a.vsh = st[15];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nsplit, (unsigned)H, (unsigned)B);
  for (int row0 = 0; row0 < Tq; row0 += kSlotRows) {  // one K / V stream per kSlotRows query rows
    const int n = Tq - row0 < kSlotRows ? Tq - row0 : kSlotRows;
    int R = 1;
    while (R < n) R *= 2;
    a.row0 = row0;
    if (D == 64) launch_extend<64>(R, grid, s, a);
    else launch_extend<128>(R, grid, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (nsplit > 1) return kfamd_attn_extend_combine(a.ws, a.o, lse, B, H, D, Tq, nsplit, ob, ot, oh, stream);
  return KFAMD_OK;
}
