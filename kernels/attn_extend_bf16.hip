// attn_extend_bf16.hip — multi-query attention over a KV cache: Tq new rows per (batch, head), split-KV.
//
// Tq (1 .. 16) query rows of one sequence, already appended to the cache [B][H][Tcap][D], attend it
// causally: row i sees keys 0 .. lens[b] - Tq + i. K and V are streamed once per (b, h, split) for up
// to 8 rows — that is the whole gain over Tq single-query launches, which stream them Tq times.
//
// Arithmetic: the VALU form of attn_decode_bf16.hip, widened to R = 1 / 2 / 4 / 8 row slots (the row count
// rounded up to a power of two; slots beyond Tq never see a valid key and are never stored). K and V go
// straight to VGPRs in 16-B loads, as in decode; every lane group (D / 8 lanes, one key row) keeps an fp32
// online softmax (m, l, o[8 dims per lane]) PER ROW SLOT and computes R dot products against each key it
// loads. Tq = 9 .. 16 runs two split launches (rows 0 .. 7, rows 8 .. Tq - 1): two streams instead of Tq.
// Sixteen row slots in one launch (16 x 8 fp32 accumulators next to 16 rows of q) exceed the 256-VGPR
// budget and spill, so that variant is not instantiated; at R = 8 the kernel takes 202 VGPRs, no spill.
// The MFMA form (16 rows fill one v_mfma_f32_16x16x32_bf16 tile for Q.K^T; P.V then needs V with keys
// along k, an LDS transpose of every V tile) was NOT built: one form serves every Tq, no cut-over.
// Measured (profiles/extend, D = 128, capacity 4096, B*H = 16 / 128, 128 .. 4096 keys) against Tq
// attention_decode calls: 1.0-1.2x at Tq = 1, 1.7-2.3x at 2, 2.8-4.5x at 4, 3.4-7.0x at 8, 3.5-7.5x at 16.
// Up to Tq = 4 it stays a KV stream (4.0-4.5 TB/s at B*H = 128, >= 2048 keys); at Tq = 8 the VALU work
// sets the time (2.1-2.3 TB/s) and Tq = 16 costs twice Tq = 8.
//
// Split structure, workspace and combine follow decode: fixed chunks of kfamd_attn_decode_split_keys()
// keys, workgroup (split, h, b) of 256 threads; with one split the block writes bf16 rows directly,
// otherwise it writes (m, l, o[D]) fp32 per row to the workspace ([B][H][Tq][nsplit]) and a second
// launch merges the splits in a fixed order (no atomics: results are bitwise repeatable).
//
// Keys at or beyond a row's limit are excluded by a branch on the key index (never multiplied by
// zero: the cache there may hold NaN); addresses are clamped to a valid key. The causal limit differs
// per row, so "no key in this split" (m = -inf, l = 0, skipped by select in every merge) happens per
// row, not only per split. The early return of an empty split is block-uniform and precedes every
// barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSplitKeys = 256;  // must equal kfamd_attn_decode_split_keys(): checked by the launcher
constexpr int kThreads = 256;
constexpr int kUnroll = 2;
constexpr int kMaxRows = 16;
constexpr int kSlotRows = 8;  // query rows per split launch (16 row slots spill: see the header)
constexpr int kMergeRows = 4;  // row slots merged per LDS pass
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ void unpack8(const u32x4& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf_lo(w[i]);
    f[2 * i + 1] = bf_hi(w[i]);
  }
}

struct ExtendArgs {
  const __bf16* q;
  const __bf16* k;
  const __bf16* v;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int H, Tq, row0, t_bound, nsplit;  // this launch holds rows row0 .. row0 + R - 1 of the Tq
  float scale_log2;
  long long qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh;
};

// workspace: [B][H][Tq][nsplit][2] (m, l) then [B][H][Tq][nsplit][D] (o), fp32
template <int D, int R>
__global__ __launch_bounds__(kThreads) void attn_extend_split(ExtendArgs a) {
  constexpr int G = D / 8;             // lanes per key row
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
    unpack8(*reinterpret_cast<const u32x4*>(a.q + b * a.qb + rr * a.qt + h * a.qh + piece * 8), qf[r]);
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[r][i] *= a.scale_log2;
    nk[r] = gr < Tq ? len - Tq + gr + 1 : 0;
  }

  const __bf16* kbase = a.k + b * a.kb + h * a.kh + piece * 8;
  const __bf16* vbase = a.v + b * a.vb + h * a.vh + piece * 8;
  const int last = k1 - 1;  // addresses are clamped to a valid key; the key index decides validity

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }

  u32x4 kn[kUnroll], vn[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int key = min(k0 + u * NG + grp, last);
    kn[u] = *reinterpret_cast<const u32x4*>(kbase + key * a.kt);
    vn[u] = *reinterpret_cast<const u32x4*>(vbase + key * a.vt);
  }
  for (int kk = k0; kk < k1; kk += KSTEP) {
    u32x4 kc[kUnroll], vc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      kc[u] = kn[u];
      vc[u] = vn[u];
    }
    if (kk + KSTEP < k1) {  // the next step's loads go out before this step's arithmetic
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int key = min(kk + KSTEP + u * NG + grp, last);
        kn[u] = *reinterpret_cast<const u32x4*>(kbase + key * a.kt);
        vn[u] = *reinterpret_cast<const u32x4*>(vbase + key * a.vt);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int key = kk + u * NG + grp;
      float kf[8], vf[8];
      unpack8(kc[u], kf);
      unpack8(vc[u], vf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) part = fmaf(qf[r][i], kf[i], part);
        const float s = kfw::group_sum<G>(part);  // every lane of the group: scale * log2e * q_r.k
        if (key < nk[r]) {                        // group-uniform; an invalid key touches no state
          const float mn = fmaxf(m[r], s);
          const float corr = exp2f(m[r] - mn);  // m = -inf on the first key: exp2(-inf) = 0
          const float p = exp2f(s - mn);
          l[r] = l[r] * corr + p;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(acc[r][i], corr, p * vf[i]);
          m[r] = mn;
        }
      }
    }
  }

  // the block's lane groups meet in LDS, RC row slots per pass
#pragma unroll
  for (int r0 = 0; r0 < R; r0 += RC) {
    if (a.row0 + r0 >= Tq) break;  // block-uniform: only padding slots are left
    if (r0 > 0) __syncthreads();  // the previous pass has been read
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

template <int D>
__global__ __launch_bounds__(D) void attn_extend_combine(const float* __restrict__ ws, __bf16* __restrict__ o,
                                                         float* __restrict__ lse, int H, int Tq, int nsplit,
                                                         long long ob, long long ot, long long oh) {
  const int h = blockIdx.x, b = blockIdx.y, r = blockIdx.z, d = threadIdx.x;
  const long long nrows = (long long)gridDim.y * H * Tq;
  const long long row = ((long long)b * H + h) * Tq + r;
  const float* ml = ws + row * nsplit * 2;
  const float* po = ws + nrows * nsplit * 2 + row * nsplit * D;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ml[2 * s]);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = ml[2 * s];
    const float w = ms == -INFINITY ? 0.f : exp2f(ms - M);  // no key of this row in the split: skipped by select
    L += ml[2 * s + 1] * w;
    O += po[s * D + d] * w;
  }
  const bool any = L > 0.f;  // no key at all
  o[b * ob + r * ot + h * oh + d] = (__bf16)(any ? O / L : 0.f);
  if (d == 0 && lse) lse[((long long)b * Tq + r) * H + h] = any ? (M + log2f(L)) * kLn2 : -INFINITY;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int D>
void launch_split(int R, dim3 grid, hipStream_t s, const ExtendArgs& a) {
  switch (R) {
    case 1: hipLaunchKernelGGL((attn_extend_split<D, 1>), grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL((attn_extend_split<D, 2>), grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL((attn_extend_split<D, 4>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((attn_extend_split<D, 8>), grid, dim3(kThreads), 0, s, a); break;
  }
}

}  // namespace

extern "C" long long kfamd_attn_extend_workspace(int B, int H, int D, int Tq, int t_bound) {
  if (Tq < 1 || Tq > kMaxRows) return 0;
  return kfamd_attn_decode_workspace(B, H, D, t_bound) * Tq;
}

// The merge of the splits' per-row records: reads only the workspace, so the FP8-cache kernel
// (attn_kv_fp8.hip) launches it too. Arguments are the caller's, already checked.
extern "C" int kfamd_attn_extend_combine(const float* ws, void* o, float* lse, int B, int H, int D, int Tq, int nsplit,
                                         long long ob, long long ot, long long oh, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 cgrid((unsigned)H, (unsigned)B, (unsigned)Tq);
  if (D == 64)
    hipLaunchKernelGGL(attn_extend_combine<64>, cgrid, dim3(64), 0, s, ws, static_cast<__bf16*>(o), lse, H, Tq, nsplit,
                       ob, ot, oh);
  else
    hipLaunchKernelGGL(attn_extend_combine<128>, cgrid, dim3(128), 0, s, ws, static_cast<__bf16*>(o), lse, H, Tq,
                       nsplit, ob, ot, oh);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

// strides (elements): q (b, t, h), k_cache (b, h, t), v_cache (b, h, t), o (b, t, h) — 12 values
extern "C" int kfamd_attn_extend_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                      float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
                                      const long long* st, void* stream) {
  if (!q || !k_cache || !v_cache || !lens || !o || !st || B <= 0 || H <= 0 || B > 65535 || H > 65535)
    return KFAMD_EINVAL;
  if ((D != 64 && D != 128) || Tq < 1 || Tq > kMaxRows || t_bound < 1) return KFAMD_EINVAL;
  if (kfamd_attn_decode_split_keys() != kSplitKeys) return KFAMD_EINVAL;
  const long long qb = st[0], qt = st[1], qh = st[2], kb = st[3], kh = st[4], kt = st[5], vb = st[6], vh = st[7],
                  vt = st[8], ob = st[9], ot = st[10], oh = st[11];
  if (kt < D || vt < D) return KFAMD_EINVAL;
  const long long lim = 1ll << 31;  // a (b, h) slice stays below 2^31 bytes
  if ((long long)t_bound * kt * 2 >= lim || (long long)t_bound * vt * 2 >= lim) return KFAMD_EINVAL;
  const int nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  if (nsplit > 1 && !ws) return KFAMD_EINVAL;
  if (!al16(q) || !al16(k_cache) || !al16(v_cache) || !al16(o) || (ws && !al16(ws))) return KFAMD_EALIGN;
  if ((qb | qt | qh | kb | kh | kt | vb | vh | vt | ob | ot | oh) & 7) return KFAMD_EALIGN;
  ExtendArgs a;
  a.q = static_cast<const __bf16*>(q);
  a.k = static_cast<const __bf16*>(k_cache);
  a.v = static_cast<const __bf16*>(v_cache);
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
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nsplit, (unsigned)H, (unsigned)B);
  for (int row0 = 0; row0 < Tq; row0 += kSlotRows) {  // one K / V stream per kSlotRows query rows
    const int n = Tq - row0 < kSlotRows ? Tq - row0 : kSlotRows;
    int R = 1;
    while (R < n) R *= 2;
    a.row0 = row0;
    if (D == 64) launch_split<64>(R, grid, s, a);
    else launch_split<128>(R, grid, s, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (nsplit > 1) return kfamd_attn_extend_combine(a.ws, a.o, lse, B, H, D, Tq, nsplit, ob, ot, oh, stream);
  return KFAMD_OK;
}
