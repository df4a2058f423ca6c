// attn_decode_bf16.hip — single-query attention over a KV cache (split-KV) and the KV append.
//
// One new query row per (batch, head) attends keys 0 .. lens[b]-1 of a cache [B][H][Tcap][D]. The
// step is a pure KV stream (2 * len * D * 2 bytes per head, 2 * len * D FLOPs): K and V go straight
// to VGPRs in 16-B loads, the dot products and P.V run on the VALU in fp32 (one query row: no MFMA
// tile to fill), cdna_hip_programming.md "Attention decode (single-token)".
//
// Split structure: the key range [0, t_bound) is cut in fixed chunks of kSplitKeys keys; workgroup
// (split, h, b) — 256 threads — walks its chunk. A key row is D / 8 lanes wide (16 B per lane), so the
// block's 256 / (D / 8) lane groups take consecutive keys (contiguous 16-B pieces across the block),
// kUnroll keys per group and step, with the next step's loads issued before the current step's
// arithmetic. Each lane group keeps its own online softmax (m, l, o[8 dims per lane]); the groups meet
// in LDS once, at the end. With one split the block writes the bf16 output directly; otherwise it
// writes (m, l, o[D]) fp32 to the workspace and a second small launch (attn_decode_combine) merges
// the splits: two dependent launches on one stream, no cross-workgroup waiting.
//
// lens is DEVICE memory: a captured step replays while the position advances. Keys >= lens[b] are
// excluded by a branch on the key index (never multiplied by zero: the cache there may hold NaN); a
// split that starts at or beyond lens[b] loads nothing and records m = -inf, l = 0, which the combine
// skips by select.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSplitKeys = 256;
constexpr int kThreads = 256;
constexpr int kUnroll = 2;
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

struct DecodeArgs {
  const __bf16* q;
  const __bf16* k;
  const __bf16* v;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int H, t_bound, nsplit;
  float scale_log2;
  long long qb, qh, kb, kh, kt, vb, vh, vt, ob, oh;
};

// workspace: [B][H][nsplit][2] (m, l) then [B][H][nsplit][D] (o), fp32
template <int D>
__global__ __launch_bounds__(kThreads) void attn_decode_split(DecodeArgs a) {
  constexpr int G = D / 8;             // lanes per key row
  constexpr int NG = kThreads / G;     // lane groups per block (= keys per block and unroll slot)
  constexpr int KSTEP = NG * kUnroll;  // keys per block step
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
  unpack8(*reinterpret_cast<const u32x4*>(a.q + b * a.qb + h * a.qh + piece * 8), qf);
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[i] *= a.scale_log2;

  const __bf16* kbase = a.k + b * a.kb + h * a.kh + piece * 8;
  const __bf16* vbase = a.v + b * a.vb + h * a.vh + piece * 8;
  const int last = k1 - 1;  // addresses are clamped to a valid key; the key index decides validity

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

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
      float kf[8];
      unpack8(kc[u], kf);
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) part = fmaf(qf[i], kf[i], part);
      const float s = kfw::group_sum<G>(part);  // every lane of the group: scale * log2e * q.k
      if (key < k1) {                           // group-uniform; an invalid key touches no state
        float vf[8];
        unpack8(vc[u], vf);
        const float mn = fmaxf(m, s);
        const float corr = exp2f(m - mn);  // m = -inf on the first key: exp2(-inf) = 0
        const float p = exp2f(s - mn);
        l = l * corr + p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(acc[i], corr, p * vf[i]);
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

template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine(const float* __restrict__ ws, __bf16* __restrict__ o,
                                                         float* __restrict__ lse, int H, int nsplit, long long ob,
                                                         long long oh) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const long long bh = (long long)b * H + h;
  const float* ml = ws + bh * nsplit * 2;
  const float* po = ws + (long long)gridDim.y * H * nsplit * 2 + bh * nsplit * D;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ml[2 * s]);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = ml[2 * s];
    const float w = ms == -INFINITY ? 0.f : exp2f(ms - M);  // an empty split: skipped by select
    L += ml[2 * s + 1] * w;
    O += po[s * D + d] * w;
  }
  const bool any = L > 0.f;  // lens[b] == 0: no key at all
  o[b * ob + h * oh + d] = (__bf16)(any ? O / L : 0.f);
  if (d == 0 && lse) lse[bh] = any ? (M + log2f(L)) * kLn2 : -INFINITY;
}

__global__ __launch_bounds__(256) void kv_append(const __bf16* __restrict__ qkv, __bf16* __restrict__ kc,
                                                 __bf16* __restrict__ vc, const int* __restrict__ pos, int B, int T,
                                                 int H, int D8, int Tcap, long long qb, long long qt, long long kb,
                                                 long long kh, long long kt, long long vb, long long vh,
                                                 long long vt) {
  const long long n = (long long)B * T * 2 * H * D8;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int d8 = (int)(r % D8);
  r /= D8;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % 2);  // 0: k, 1: v
  r /= 2;
  const int t = (int)(r % T);
  const int b = (int)(r / T);
  const long long row = (long long)pos[b] + t;
  if (row < 0 || row >= Tcap) return;  // past the capacity: dropped, never written
  const u32x4 val =
      *reinterpret_cast<const u32x4*>(qkv + b * qb + t * qt + ((long long)(s + 1) * H + h) * (D8 * 8) + d8 * 8);
  __bf16* dst = s == 0 ? kc + b * kb + h * kh + row * kt : vc + b * vb + h * vh + row * vt;
  *reinterpret_cast<u32x4*>(dst + d8 * 8) = val;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int kfamd_attn_decode_split_keys(void) { return kSplitKeys; }

extern "C" long long kfamd_attn_decode_workspace(int B, int H, int D, int t_bound) {
  if (B <= 0 || H <= 0 || (D != 64 && D != 128) || t_bound < 1) return 0;
  const long long nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  return (long long)B * H * nsplit * (D + 2) * (long long)sizeof(float);
}

// The merge of the splits' (m, l, o[D]) fp32 records into bf16 rows: reads only the workspace, so the
// FP8-cache kernels (attn_kv_fp8.hip) launch it too. Arguments are the caller's, already checked.
extern "C" int kfamd_attn_decode_combine(const float* ws, void* o, float* lse, int B, int H, int D, int nsplit,
                                         long long ob, long long oh, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 cgrid((unsigned)H, (unsigned)B);
  if (D == 64)
    hipLaunchKernelGGL(attn_decode_combine<64>, cgrid, dim3(64), 0, s, ws, static_cast<__bf16*>(o), lse, H, nsplit, ob,
                       oh);
  else
    hipLaunchKernelGGL(attn_decode_combine<128>, cgrid, dim3(128), 0, s, ws, static_cast<__bf16*>(o), lse, H, nsplit,
                       ob, oh);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

// strides (elements): q (b, h), k_cache (b, h, t), v_cache (b, h, t), o (b, h) — 10 values
extern "C" int kfamd_attn_decode_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                      float* lse, void* ws, int B, int H, int D, int t_bound, float scale,
                                      const long long* st, void* stream) {
  if (!q || !k_cache || !v_cache || !lens || !o || !st || B <= 0 || H <= 0 || B > 65535 || H > 65535)
    return KFAMD_EINVAL;
  if ((D != 64 && D != 128) || t_bound < 1) return KFAMD_EINVAL;
  const long long qb = st[0], qh = st[1], kb = st[2], kh = st[3], kt = st[4], vb = st[5], vh = st[6], vt = st[7],
                  ob = st[8], oh = st[9];
  if (kt < D || vt < D) return KFAMD_EINVAL;
  const long long lim = 1ll << 31;  // a (b, h) slice stays below 2^31 bytes
  if ((long long)t_bound * kt * 2 >= lim || (long long)t_bound * vt * 2 >= lim) return KFAMD_EINVAL;
  const int nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  if (nsplit > 1 && !ws) return KFAMD_EINVAL;
  if (!al16(q) || !al16(k_cache) || !al16(v_cache) || !al16(o) || (ws && !al16(ws))) return KFAMD_EALIGN;
  if ((qb | qh | kb | kh | kt | vb | vh | vt | ob | oh) & 7) return KFAMD_EALIGN;
  DecodeArgs a;
  a.q = static_cast<const __bf16*>(q);
  a.k = static_cast<const __bf16*>(k_cache);
  a.v = static_cast<const __bf16*>(v_cache);
  a.lens = lens;
  a.o = static_cast<__bf16*>(o);
  a.lse = lse;
  a.ws = static_cast<float*>(ws);
  a.H = H;
  a.t_bound = t_bound;
  a.nsplit = nsplit;
  a.scale_log2 = scale * kLog2e;
  a.qb = qb, a.qh = qh, a.kb = kb, a.kh = kh, a.kt = kt, a.vb = vb, a.vh = vh, a.vt = vt, a.ob = ob, a.oh = oh;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nsplit, (unsigned)H, (unsigned)B);
  if (D == 64) hipLaunchKernelGGL(attn_decode_split<64>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(attn_decode_split<128>, grid, dim3(kThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (nsplit > 1) return kfamd_attn_decode_combine(a.ws, a.o, lse, B, H, D, nsplit, ob, oh, stream);
  return KFAMD_OK;
}

// K and V rows of a fused QKV activation [B][T][3][H][D] (element strides qb, qt; [3][H][D] dense)
// into the caches [B][H][Tcap][D] (strides b, h, t) at rows pos[b] .. pos[b] + T - 1. pos: device
// int32 [B], not advanced here. Rows at or beyond Tcap are dropped.
extern "C" int kfamd_kv_append_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int H,
                                    int D, int Tcap, long long qb, long long qt, const long long* cache_strides,
                                    void* stream) {
  if (!qkv || !k_cache || !v_cache || !pos || !cache_strides || B <= 0 || T <= 0 || H <= 0 || D <= 0 || D % 8 ||
      Tcap <= 0)
    return KFAMD_EINVAL;
  const long long* c = cache_strides;
  if (!al16(qkv) || !al16(k_cache) || !al16(v_cache)) return KFAMD_EALIGN;
  if ((qb | qt | c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & 7) return KFAMD_EALIGN;
  const long long n = (long long)B * T * 2 * H * (D / 8);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  hipLaunchKernelGGL(kv_append, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const __bf16*>(qkv), static_cast<__bf16*>(k_cache), static_cast<__bf16*>(v_cache), pos,
                     B, T, H, D / 8, Tcap, qb, qt, c[0], c[1], c[2], c[3], c[4], c[5]);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}
