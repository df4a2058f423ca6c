// sample_bf16.hip — one token per row of bf16 logits: greedy, temperature, top-k, top-p, stop token
// (kubeflow_rm_amd.ops.sample; the rule is stated at kfamd_sample_bf16 in kfamd_kernels.h).
//
// One 1024-thread workgroup per row; wave w owns the contiguous index segment [w * seg, (w + 1) * seg)
// and walks it 64 tokens at a time (coalesced 2-byte loads, no alignment assumed). The row comes from
// HBM once, in the first pass; the later passes re-read it from L2 (V <= 2^20 is at most 2 MiB, and one
// code path serves every V: there is no staging cut-over).
//
// Order without a sort: a bf16 logit maps to a 16-bit key that grows with its value, so the top-k cut is
// a two-level radix select on key counts (high byte, then low byte inside the bin that holds the cut),
// and the tie group at the cut admits its lowest indices first through a rank that an index-order pass
// counts with ballots.
//
// Mass without a rounding order: w = exp2((x - x_max) * inv_temp * log2 e) is evaluated in fp32 and
// stored as a 64-bit fixed-point number in units of 2^-40 (w <= 1 and V <= 2^20, so no sum passes 2^60).
// Equal keys give equal weights, so the mass of a key is count * weight, and every sum — histogram bins
// (LDS integer atomics), wave and block totals, the running sum of the draw — is an integer sum: exact,
// independent of the order of the additions, and no chain of fp32 additions exists at all. What is
// left of the tolerance is the fp32 exponential (better than 2^-17 relative) and the 2^-40 quantum
// (2^-20 of the mass over 2^20 terms). The kept mass W the histograms predict is exactly what the
// index-order pass sums, so floor(u * W) always falls inside a kept token's interval.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kMaxV = 1 << 20;
constexpr float kFixOne = 0x1p40f;  // fixed-point one
constexpr unsigned kNoLimit = 0xFFFFFFFFu;

// -0 counts as +0: equal logits must get equal keys
__device__ __forceinline__ unsigned canon_bits(unsigned short b) { return b == 0x8000u ? 0u : b; }
// 16-bit key, monotone in the value (negative values: all bits flipped; others: sign bit set)
__device__ __forceinline__ unsigned key_of(unsigned b) { return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u); }
__device__ __forceinline__ unsigned bits_of(unsigned key) { return (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu); }
__device__ __forceinline__ float value_of(unsigned key) { return __uint_as_float(bits_of(key) << 16); }
// the weight of a key in units of 2^-40: a pure function of the key, so ties weigh the same
__device__ __forceinline__ u64 weight_of(unsigned key, float xmax, float c) {
  return (u64)(__builtin_amdgcn_exp2f((value_of(key) - xmax) * c) * kFixOne);
}

struct Shared {
  float red[kWaves];
  unsigned cnt1[256];  // tokens per high key byte
  u64 mass1[256];      // their mass
  unsigned cnt2[256];  // tokens per low key byte inside one high bin
  unsigned wave_ties[kWaves];
  u64 wave_mass[kWaves];
  // results of the bin searches (written by one lane of wave 0, read by everyone after a barrier)
  int bin;
  unsigned above_cnt;
  u64 above_mass, total_mass;
};

__device__ __forceinline__ float block_max(float v, Shared& sh) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  v = kfw::wave_max(v);
  if (l == 0) sh.red[w] = v;
  __syncthreads();
  float r = sh.red[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) r = fmaxf(r, sh.red[k]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Wave 0 searches 256 bins in descending bin order: lane l owns bins 255 - 4l .. 252 - 4l with the counts
// c[i] and masses m[i]. The first bin whose inclusive prefix (count, or mass with BY_MASS) reaches
// `target` goes to sh.bin with the count and mass of the bins above it; the last bin if none does.
// sh.total_mass gets the mass of all 256 bins.
template <bool BY_MASS>
__device__ __forceinline__ void wave0_find(const unsigned (&c)[4], const u64 (&m)[4], u64 target, Shared& sh) {
  const int lane = threadIdx.x & 63;
  unsigned pc[4];
  u64 pm[4];
  pc[0] = c[0];
  pm[0] = m[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) { pc[i] = pc[i - 1] + c[i]; pm[i] = pm[i - 1] + m[i]; }
  unsigned ic = pc[3];
  u64 im = pm[3];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned oc = __shfl_up(ic, d);
    const u64 om = __shfl_up(im, d);
    if (lane >= d) { ic += oc; im += om; }
  }
  const unsigned ec = ic - pc[3];
  const u64 em = im - pm[3];
  int hit = -1;
  unsigned hc = ec + pc[2];  // what lies above the lane's last bin: lane 63's answer when no bin reaches
  u64 hm = em + pm[2];
#pragma unroll
  for (int i = 3; i >= 0; --i)
    if ((BY_MASS ? em + pm[i] : (u64)(ec + pc[i])) >= target) {
      hit = i;
      hc = ec + pc[i] - c[i];
      hm = em + pm[i] - m[i];
    }
  const u64 lanes = __ballot(hit >= 0);
  const int first = lanes ? __ffsll((long long)lanes) - 1 : 63;
  if (!lanes) hit = 3;
  if (lane == first) {
    sh.bin = 255 - 4 * lane - hit;
    sh.above_cnt = hc;
    sh.above_mass = hm;
  }
  if (lane == 63) sh.total_mass = im;
}

struct Params {
  const unsigned short* logits;
  long long ld;
  const float* u;
  const int* step;
  long long* out;
  long long* seq;
  long long seq_ld;
  int* done;
  int B, V, S;
  float inv_temp;
  int top_k;
  float top_p;
  long long stop_token;
};

__global__ __launch_bounds__(kThreads) void sample_row(const Params p) {
  __shared__ Shared sh;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int V = p.V;
  const int s = p.step ? *p.step : 0;
  if (s < 0 || s >= p.S) return;  // the uniforms and the sequence column of this step do not exist
  const bool stop = p.stop_token >= 0 && p.done != nullptr;
  if (stop && p.done[b] != 0) {  // a finished row: pad
    if (tid == 0) {
      p.out[b] = p.stop_token;
      if (p.seq) p.seq[b * p.seq_ld + s] = p.stop_token;
    }
    return;
  }
  const unsigned short* x = p.logits + b * p.ld;
  const int seg = (((V + kWaves - 1) / kWaves) + 63) & ~63;  // tokens per wave, whole 64-token steps
  const int lo = wave * seg, hi = min(V, lo + seg);

  // ---- pass 0: the largest key and its lowest index (the row's only trip to HBM) ----
  unsigned bk = 0;
  int bi = kMaxV;
  for (int base = lo; base < hi; base += 64) {
    const int j = base + lane;
    if (j < hi) {
      const unsigned k = key_of(canon_bits(x[j]));
      if (k > bk || bi == kMaxV) { bk = k; bi = j; }
    }
  }
  const unsigned kmax = (unsigned)block_max((float)bk, sh);  // 16-bit keys and indices < 2^20: exact in fp32
  const int imax = (int)-block_max((bi < kMaxV && bk == kmax) ? -(float)bi : -(float)kMaxV, sh);

  long long token = -1;  // set by the one thread that emits
  const bool greedy = p.inv_temp == 0.f || p.top_k == 1;
  if (greedy) {
    if (tid == 0) token = imax;
  } else {
    const float xmax = value_of(kmax);
    const float c = p.inv_temp * 1.44269504088896341f;
    const unsigned K = (p.top_k > 0 && p.top_k < V) ? (unsigned)p.top_k : 0u;  // 0: no top-k cut
    const bool need_k = K != 0, need_p = p.top_p < 1.f;
    unsigned cut_key = 0, cut_adm = kNoLimit;  // kept: key > cut_key, or key == cut_key with tie rank < cut_adm

    if (need_k || need_p) {
      // ---- level 1: tokens (and mass) per high key byte ----
      if (tid < 256) { sh.cnt1[tid] = 0; sh.mass1[tid] = 0; }
      __syncthreads();
      for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        if (j < hi) {
          const unsigned k = key_of(canon_bits(x[j]));
          atomicAdd(&sh.cnt1[k >> 8], 1u);
          if (need_p) atomicAdd(&sh.mass1[k >> 8], weight_of(k, xmax, c));
        }
      }
      __syncthreads();

      int Hk = -1;            // the high bin that holds the top-k cut
      unsigned ck = 0, ak = kNoLimit;
      u64 mass_above_hk = 0;  // mass of the bins above Hk
      u64 Zk = 0;             // mass of the top-k set (needed by top-p only)
      if (need_k) {
        if (wave == 0) {
          unsigned cc[4];
          u64 mm[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { cc[i] = sh.cnt1[255 - 4 * lane - i]; mm[i] = sh.mass1[255 - 4 * lane - i]; }
          wave0_find<false>(cc, mm, K, sh);
        }
        __syncthreads();
        Hk = sh.bin;
        const unsigned cnt_above_hk = sh.above_cnt;
        mass_above_hk = sh.above_mass;
        // ---- level 2: tokens per low key byte inside Hk ----
        if (tid < 256) sh.cnt2[tid] = 0;
        __syncthreads();
        for (int base = lo; base < hi; base += 64) {
          const int j = base + lane;
          if (j < hi) {
            const unsigned k = key_of(canon_bits(x[j]));
            if ((int)(k >> 8) == Hk) atomicAdd(&sh.cnt2[k & 255], 1u);
          }
        }
        __syncthreads();
        if (wave == 0) {
          unsigned cc[4];
          u64 mm[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int l2 = 255 - 4 * lane - i;
            cc[i] = sh.cnt2[l2];
            mm[i] = cc[i] * weight_of((unsigned)(Hk << 8 | l2), xmax, c);
          }
          wave0_find<false>(cc, mm, K - cnt_above_hk, sh);
        }
        __syncthreads();
        ck = (unsigned)(Hk << 8 | sh.bin);
        ak = K - cnt_above_hk - sh.above_cnt;  // members of the tie group at ck inside the top k
        Zk = mass_above_hk + sh.above_mass + ak * weight_of(ck, xmax, c);
        cut_key = ck;
        cut_adm = ak;
        __syncthreads();  // sh.bin / above_* are rewritten below
      }

      if (need_p) {
        // own masses of the high bins, restricted to the top-k set
        unsigned cc[4] = {0, 0, 0, 0};
        u64 mm[4] = {0, 0, 0, 0};
        if (wave == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h = 255 - 4 * lane - i;
            mm[i] = !need_k ? sh.mass1[h] : h > Hk ? sh.mass1[h] : h == Hk ? Zk - mass_above_hk : 0;
          }
          if (!need_k) wave0_find<true>(cc, mm, ~0ull, sh);  // the total mass only
        }
        if (!need_k) {
          __syncthreads();
          Zk = sh.total_mass;
          __syncthreads();
        }
        // the mass the kept prefix must reach: ceil(top_p * Zk), in [1, Zk]
        u64 Tp = (u64)ceil((double)p.top_p * (double)Zk);
        Tp = Tp < 1 ? 1 : Tp > Zk ? Zk : Tp;
        if (wave == 0) wave0_find<true>(cc, mm, Tp, sh);
        __syncthreads();
        const int Hp = sh.bin;
        const u64 mass_above_hp = sh.above_mass;
        __syncthreads();
        if (Hp != Hk) {  // cnt2 holds another bin (or nothing): count Hp's low bytes
          if (tid < 256) sh.cnt2[tid] = 0;
          __syncthreads();
          for (int base = lo; base < hi; base += 64) {
            const int j = base + lane;
            if (j < hi) {
              const unsigned k = key_of(canon_bits(x[j]));
              if ((int)(k >> 8) == Hp) atomicAdd(&sh.cnt2[k & 255], 1u);
            }
          }
          __syncthreads();
        }
        if (wave == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned k = (unsigned)(Hp << 8 | (255 - 4 * lane - i));
            unsigned n = sh.cnt2[255 - 4 * lane - i];
            if (need_k && k < ck) n = 0;
            if (need_k && k == ck) n = ak;
            cc[i] = n;
            mm[i] = n * weight_of(k, xmax, c);
          }
          wave0_find<true>(cc, mm, Tp - mass_above_hp, sh);
        }
        __syncthreads();
        const unsigned cp = (unsigned)(Hp << 8 | sh.bin);
        const u64 wq = weight_of(cp, xmax, c);
        unsigned avail = sh.cnt2[sh.bin];
        if (need_k && cp == ck) avail = ak;
        const u64 want = Tp - mass_above_hp - sh.above_mass;  // mass the tie group at cp has to supply
        u64 np = wq ? (want + wq - 1) / wq : avail;
        np = np < 1 ? 1 : np > avail ? avail : np;
        cut_key = cp;
        cut_adm = (unsigned)np;
      }
    }

    // ---- index order: tie ranks, the kept mass per wave, then the draw ----
    unsigned tie_base = 0;
    if (cut_adm != kNoLimit) {
      unsigned n = 0;
      for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const bool tie = j < hi && key_of(canon_bits(x[j])) == cut_key;
        n += __popcll(__ballot(tie));
      }
      if (lane == 0) sh.wave_ties[wave] = n;
      __syncthreads();
      for (int w = 0; w < wave; ++w) tie_base += sh.wave_ties[w];
    }
    const u64 lanes_below = (1ull << lane) - 1;
    {
      u64 acc = 0;
      unsigned rank0 = tie_base;
      for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const bool in = j < hi;
        const unsigned k = in ? key_of(canon_bits(x[j])) : 0u;
        const bool tie = in && k == cut_key;
        const u64 ties = __ballot(tie);
        const bool kept = in && (k > cut_key || (tie && rank0 + __popcll(ties & lanes_below) < cut_adm));
        if (kept) acc += weight_of(k, xmax, c);
        rank0 += __popcll(ties);
      }
      acc = wave_sum_u64(acc);
      if (lane == 0) sh.wave_mass[wave] = acc;
    }
    __syncthreads();
    u64 W = 0, before = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) before = W;
      W += sh.wave_mass[w];
    }
    // floor(u * W) with u cut to 24 fractional bits: below W, so some kept token's interval holds it
    float uf = p.u[(long long)s * p.B + b];
    uf = uf < 0.f ? 0.f : uf;
    u64 uq = (u64)(uf * 0x1p24f);
    uq = uq > 0xFFFFFFull ? 0xFFFFFFull : uq;
    const u64 Tq = __umul64hi(W, uq << 40);
    if (W == 0) {  // out of contract (no finite logit); stay defined
      if (tid == 0) token = imax;
    } else if (before <= Tq && Tq < before + sh.wave_mass[wave]) {  // exactly one wave
      u64 run = before;
      unsigned rank0 = tie_base;
      for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const bool in = j < hi;
        const unsigned k = in ? key_of(canon_bits(x[j])) : 0u;
        const bool tie = in && k == cut_key;
        const u64 ties = __ballot(tie);
        const bool kept = in && (k > cut_key || (tie && rank0 + __popcll(ties & lanes_below) < cut_adm));
        rank0 += __popcll(ties);
        u64 inc = kept ? weight_of(k, xmax, c) : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const u64 o = __shfl_up(inc, d);
          if (lane >= d) inc += o;
        }
        const u64 hits = __ballot(run + inc > Tq);
        if (hits) {
          if (lane == __ffsll((long long)hits) - 1) token = j;
          break;
        }
        run += __shfl(inc, 63);
      }
    }
  }

  if (token >= 0) {
    p.out[b] = token;
    if (p.seq) p.seq[b * p.seq_ld + s] = token;
    if (stop && token == p.stop_token) p.done[b] = 1;
  }
}

}  // namespace

extern "C" int kfamd_sample_bf16(const void* logits, long long ld, const float* u, const int* step, long long* out,
                                 long long* seq, long long seq_ld, int* done, int B, int V, int S, float inv_temp,
                                 int top_k, float top_p, long long stop_token, void* stream) {
  if (!logits || !u || !out || B < 1 || V < 1 || V > kMaxV || S < 1) return KFAMD_EINVAL;
  if ((reinterpret_cast<uintptr_t>(logits) & 1) || (B > 1 && ld < V)) return KFAMD_EINVAL;
  if (!(inv_temp >= 0.f) || !isfinite(inv_temp) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) return KFAMD_EINVAL;
  if (seq && seq_ld < S) return KFAMD_EINVAL;
  if ((stop_token >= 0) != (done != nullptr) || stop_token >= V) return KFAMD_EINVAL;
  Params p{static_cast<const unsigned short*>(logits), ld, u, step, out, seq, seq_ld, done, B, V, S, inv_temp, top_k,
           top_p, stop_token};
  hipLaunchKernelGGL(sample_row, dim3(B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}
