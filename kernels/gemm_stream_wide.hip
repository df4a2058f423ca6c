// gemm_stream_wide.hip — weight-streaming NT GEMM for decode steps of 17 to 128 rows (1 <= M <= 128 in contract):
//   C[M][N] = act(alpha * wscale[n] * (A[M][K] . W[N][K]^T) + bias[n]) (+ R[M][N]),
// and the gated (SwiGLU) form over interleaved gate / up rows (ops/swiglu.py's layout rule). A, bias, R, C are bf16,
// accumulation fp32. W is bf16, OCP e4m3fn codes with one fp32 scale per row (ops.QuantizedWeight) or MXFP4
// (ops.MXFP4Weight, whose docstring is the format rule; no row scale: code x group scale is an exact bf16). At M
// rows a GEMM does about M FLOP per weight byte, far below the chip's ridge: like the M <= 16 kernels
// (gemm_skinny_*.hip) this one is a single pass over the weights, but with its own MFMA mapping, because their form
// (8 weight rows twice in the 16-row operand, activations clamped to 16 columns) cannot hold more than 16 rows.
//
// One template, stream_wide<F, MB, TILES, GLU>, over the weight format F (a loader trait: 16 bytes of a weight row
// -> NF = 1 / 2 / 4 bf16x8 operand fragments for bf16 / FP8 / MXFP4; the widening functions are those of
// gemm_skinny_w8.hip and gemm_skinny_mx4.hip, re-stated), the activation row blocks MB = ceil(M / 16) rounded up to
// 2 / 4 / 8, and the 16-row weight tiles per workgroup TILES = 1 / 2 / 4.
//   MFMA mapping: v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the 16-row operand (16 distinct weight rows: operand
//     row r = lane & 15, k-slot q = lane >> 4) and the activations as the 16-column operand. A weight fragment is
//     loaded from HBM once and multiplied with the MB activation fragments into MB f32x4 accumulators per tile, all in
//     registers (MB x TILES x 4: at most 128, AGPRs). Activation rows at or beyond M are clamped to row M - 1 and
//     never stored; a result column depends on its own activation row only.
//   Work split: a 256-thread workgroup owns TILES x 16 weight rows and splits K over its 4 waves in chunks of 128
//     weight BYTES per row (64 bf16, 128 FP8 or 256 MXFP4 elements): wave w takes chunks w, w + 4, ... . A chunk is two
//     steps; in step s lane (r, q) loads the 16-B piece 4 s + q of row r's chunk, so one load instruction covers 64
//     contiguous bytes of each of 16 rows and the two steps a whole 128-B line. The k order inside an MFMA is whatever
//     this gives: k-slot q of fragment f of step s is elements 8 f .. 8 f + 7 of piece 4 s + q, and the activation
//     fragment is read from the same elements (EPP = 8 NF contiguous elements of the row per lane and piece).
//   Weight loads: HBM -> VGPRs in 16-B pieces, no LDS. A wave keeps U = 4 / TILES chunks of every tile in flight
//     (U x 2 x TILES = 8 pieces, 32 KB per workgroup) and loads the NEXT group of chunks before it computes on the
//     current one (two register sets, the loop unrolled twice so that no set is copied): the HBM latency is under
//     the MFMAs and the activation loads of a whole group, not only under other waves.
//   Activations: straight from L2 to registers, not through LDS. A wave's K slice is its own, so LDS would buy reuse
//     across TILES only, which the registers already give: an activation fragment is loaded once per (chunk, step,
//     fragment, row block) and used against all TILES weight fragments. Every workgroup reads all of A once: L2
//     traffic is M / (16 TILES) times the weight bytes, which is what TILES > 1 is for. The loads run one stage ahead
//     of the MFMAs (a stage is up to 8 pieces: all MB row blocks of max(1, 8 / MB) fragments; two buffers).
//   K tail: K % EPP == 0 (the formats' contracts: 8 / 16 / 32), so a piece lies wholly inside or outside K. An outside
//     weight piece is zero (its address clamped to the row's start); the activation piece then read is the row's
//     first (finite in, exact zero products out).
//   Reduction: per row block the four waves' partials meet in LDS (two 4 x TILES x 1 KB buffers, one barrier per
//     block) and wave (block & 3) sums them in wave order 0, 1, 2, 3: no atomics, deterministic, a captured launch
//     replays bit for bit. In the 16x16 result layout a lane holds weight rows 4 q .. 4 q + 3 of activation row r:
//     a (gate, up) pair sits in one lane and the gated epilogue needs no exchange; the plain epilogue (alpha x row
//     scale, bias, activation code, residual, ONE rounding to bf16) stores the four as one 8-byte store where C
//     allows (C 8-B aligned, ldc % 4 == 0), else element by element. Rows of the last tile are clamped and
//     store-masked: any N.
//
// Cut-overs (kfamd_gemm_nt_stream_*, tiles = 0; choose_tiles). Measured with every tiles value forced on the gpt-1b
// shapes at M = 17, 32, 64, 128 (tools/decode_bench.py --steps stream, profiles/stream/README.md; medians of 7
// interleaved blocks, weights rotated past the last-level cache, us per call from Python, about 10.5 us the launch
// floor), TILES 1 / 2 / 4, against variant "auto" on bf16 at the same M:
//   2048x2048   bf16 M = 32 11.0 / 13.5 / 20.4, M = 128 25.3 / 33.8 / 51.2; MXFP4 M = 32 12.7 / 10.9 / 15.6, M = 128
//               38.5 / 30.2 / 44.5; auto 80.5 (M = 32), 18.2 (M = 128)
//   6144x2048   bf16 M = 32 17.1 / 15.2 / 21.8, M = 64 26.7 / 22.4 / 34.0; FP8 M = 32 14.3 / 12.3 / 19.5; MXFP4 M = 32
//               21.8 / 11.1 / 15.6, M = 64 40.2 / 17.3 / 25.5; auto 85.5 (M = 32), 79.9 (M = 64), 26.7 (M = 128)
//   8192x2048   bf16 M = 32 17.9 / 16.0 / 22.5; FP8 14.4 / 12.7 / 19.8; MXFP4 22.8 / 11.4 / 16.2; auto 85.7
//   2048x8192   bf16 M = 32 28.3 / 40.6 / 59.9, M = 64 44.9 / 58.4 / 91.4; FP8 M = 32 23.9 / 28.5 / 47.8; MXFP4 M = 32
//               24.7 / 28.9 / 40.9; auto 311.6 (M = 32), 40.4 (M = 64), 23.2 (M = 128)
//   32000x2048  bf16 M = 32 56.2 / 50.5 / 40.8, M = 128 159.7 / 137.7 / 122.9; FP8 M = 32 46.8 / 37.6 / 28.7; MXFP4
//               M = 32 78.1 / 34.0 / 26.2; auto 42.7 (M = 32), 43.6 (M = 64), 34.3 (M = 128)
//   16384x2048 gated  bf16 M = 32 31.2 / 24.5 / 23.2, M = 128 80.8 / 63.5 / 48.2; MXFP4 M = 32 41.2 / 17.5 / 15.2;
//               GEMM + gate kernel 50.5 (M = 32), 32.1 (M = 128)
// Hence TILES = 4 from N = 16384, 2 from N = 4096, 1 below; MXFP4 takes 2 at narrow N too (its TILES = 1 form pays a
// scale byte load per piece against one tile) except on a long K (2048x8192), where 64 workgroups are too few. What the
// design does not reach: from M = 64 the time follows the activation traffic from L2, M / (16 TILES) times the weight
// bytes, not the weight bytes (the three formats level, doubling M doubles the time), and "auto" wins every shape at
// M = 128 and the LM head from M = 64; TILES = 1 under-fills N = 2048 (128 workgroups) and the 8-row split of the tile
// was not tried. GPT's stream_rows therefore defaults to 16 and 64 is the recommended value.
//
// Registers (gfx950, -Rpass-analysis=kernel-resource-usage; 0 scratch bytes in every instantiation, which the build
// checks; VGPRs / AGPRs, bf16 / FP8 / MXFP4, the gated forms within 9): <2, 1> 144 / 16, 134 / 20, 152 / 16; <4, 2>
// 111 / 76, 102 / 80, 111 / 80; <8, 4> 242 / 256, 249 / 256, 235 / 256 (one workgroup per CU).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxM = 128;

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case KFAMD_ACT_RELU: return v > 0.f ? v : 0.f;
    case KFAMD_ACT_GELU_TANH: {
      const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
      return 0.5f * v * (1.f + tanhf(u));
    }
    case KFAMD_ACT_SILU: return v / (1.f + __expf(-v));
    default: return v;
  }
}

// ---- the weight formats: 16 bytes of a weight row -> NF bf16x8 fragments (fragment f: elements 8 f .. 8 f + 7) ----
struct Bf16Weight {
  static constexpr int NF = 1;
  static constexpr bool kGroupScale = false, kRowScale = false;
  static __device__ __forceinline__ bf16x8 frag(const u32x4& p, int, unsigned) { return __builtin_bit_cast(bf16x8, p); }
};

// e4m3fn codes (gemm_skinny_w8.hip's widening): v_cvt_pk_f32_fp8, then the upper halves of two fp32 (their lower
// halves are zero) packed into a bf16 pair by v_perm_b32: exact
struct Fp8Weight {
  static constexpr int NF = 2;
  static constexpr bool kGroupScale = false, kRowScale = true;
  static __device__ __forceinline__ bf16x8 frag(const u32x4& p, int f, unsigned) {
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int w = (int)p[2 * f + h];
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
      o[2 * h] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
      o[2 * h + 1] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
    }
    return __builtin_bit_cast(bf16x8, o);
  }
};

// MXFP4 (gemm_skinny_mx4.hip's widening): a piece is one whole MX group, 32 codes and one e8m0 scale byte e;
// v_cvt_scalef32_pk_bf16_fp4 turns one byte and the fp32 scale (e << 23) into a bf16 pair, low nibble first
struct Mx4Weight {
  static constexpr int NF = 4;
  static constexpr bool kGroupScale = true, kRowScale = false;
  static __device__ __forceinline__ bf16x8 frag(const u32x4& p, int f, unsigned e) {
    const float s = __uint_as_float(e << 23);
    const unsigned w = p[f];
    const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0);
    const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
    const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2);
    const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
    return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  }
};

struct StreamArgs {
  const __bf16* A;
  const uint8_t* W;      // weight rows, ldw BYTES apart: bf16 elements, e4m3fn codes or e2m1 code pairs
  const uint8_t* S;      // MXFP4: e8m0 scales [N][lds]
  const float* wscale;   // FP8: [N]
  __bf16* C;
  const __bf16* bias;
  const __bf16* R;
  int M, N, K;
  long long lda, ldw, lds, ldc, ldr;
  float alpha;
  int act;
  int vec;  // C rows take 8-byte stores at columns that are multiples of 4
};

// the weight pieces (and MXFP4 scale bytes) of one group of U chunks: raw load results, masked where they are used
template <int U, int TILES>
struct WeightSet {
  u32x4 w[U][2][TILES];
  unsigned e[U][2][TILES];
};

template <class F, int MB, int TILES, bool GLU>
__global__ __launch_bounds__(256) void stream_wide(StreamArgs a) {
  constexpr int NF = F::NF, EPP = 8 * NF;  // fragments / elements per 16-B weight piece
  constexpr int U = 4 / TILES;             // chunks per group (header comment)
  constexpr int FG = NF < (MB >= 8 ? 1 : 8 / MB) ? NF : (MB >= 8 ? 1 : 8 / MB);  // fragments per activation stage
  constexpr int NFG = NF / FG;
  constexpr int NSTAGE = U * 2 * NFG;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * (16 * TILES);
  const int pieces = a.K / EPP;
  const int nchunks = (pieces + 7) / 8;

  const uint8_t *wrow[TILES], *srow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const long long row = min(n0 + t * 16 + r, a.N - 1);
    wrow[t] = a.W + row * a.ldw;
    srow[t] = F::kGroupScale ? a.S + row * a.lds : nullptr;
  }
  const __bf16* arow[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) arow[mb] = a.A + (long long)min(mb * 16 + r, a.M - 1) * a.lda;

  f32x4 acc[MB][TILES];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int t = 0; t < TILES; ++t) acc[mb][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the piece a lane takes in step s of the group's chunk u (first chunk c0): pieces of a row, 16 B each
  auto piece = [&](int c0, int u, int s) __attribute__((always_inline)) { return (c0 + 4 * u) * 8 + s * 4 + q; };

  auto load_weights = [&](WeightSet<U, TILES>& ws, int c0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int p = piece(c0, u, s);
        const int pc = p < pieces ? p : 0;  // a clamped (valid) address; the piece is zeroed where it is used
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          ws.w[u][s][t] = *reinterpret_cast<const u32x4*>(wrow[t] + (long long)pc * 16);
          if constexpr (F::kGroupScale) ws.e[u][s][t] = srow[t][pc];
        }
      }
  };

  // one group: NSTAGE stages of activation loads, each issued one stage ahead of its MFMAs
  auto compute = [&](const WeightSet<U, TILES>& ws, int c0) __attribute__((always_inline)) {
    u32x4 x[2][MB * FG];
    auto load_x = [&](int st, u32x4* xb) __attribute__((always_inline)) {
      const int fg = st % NFG, s = (st / NFG) & 1, u = st / (2 * NFG);
      const int p = piece(c0, u, s);
      const long long k0 = p < pieces ? (long long)p * EPP : 0;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int ff = 0; ff < FG; ++ff)
          xb[mb * FG + ff] = *reinterpret_cast<const u32x4*>(arow[mb] + k0 + (fg * FG + ff) * 8);
    };
    load_x(0, x[0]);
#pragma unroll
    for (int st = 0; st < NSTAGE; ++st) {
      if (st + 1 < NSTAGE) load_x(st + 1, x[(st + 1) & 1]);
      const int fg = st % NFG, s = (st / NFG) & 1, u = st / (2 * NFG);
      const bool ok = piece(c0, u, s) < pieces;
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        u32x4 w = ws.w[u][s][t];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = ok ? w[i] : 0u;
#pragma unroll
        for (int ff = 0; ff < FG; ++ff) {
          const bf16x8 f = F::frag(w, fg * FG + ff, F::kGroupScale ? ws.e[u][s][t] : 0u);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
            acc[mb][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                f, __builtin_bit_cast(bf16x8, x[st & 1][mb * FG + ff]), acc[mb][t], 0, 0, 0);
        }
      }
    }
  };

  {
    WeightSet<U, TILES> wa, wb;
    int c0 = wave;
    load_weights(wa, c0);
    while (c0 < nchunks) {  // wave-uniform
      load_weights(wb, c0 + 4 * U);
      compute(wa, c0);
      c0 += 4 * U;
      if (c0 >= nchunks) break;
      load_weights(wa, c0 + 4 * U);
      compute(wb, c0);
      c0 += 4 * U;
    }
  }

  // reduction over the waves and epilogue, row block by row block. acc[mb][t][i]: activation row 16 mb + r, weight
  // row n0 + 16 t + 4 q + i.
  __shared__ f32x4 red[2][4][TILES][64];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (mb * 16 >= a.M) break;  // kernel-uniform
#pragma unroll
    for (int t = 0; t < TILES; ++t) red[mb & 1][wave][t][lane] = acc[mb][t];
    __syncthreads();
    if (wave != (mb & 3)) continue;
    const int m = mb * 16 + r;
    if (m >= a.M) continue;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const int nb = n0 + t * 16 + 4 * q;
      if (nb >= a.N) continue;
      const f32x4 sum = ((red[mb & 1][0][t][lane] + red[mb & 1][1][t][lane]) + red[mb & 1][2][t][lane]) +
                        red[mb & 1][3][t][lane];
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = min(nb + i, a.N - 1);
        v[i] = sum[i] * (F::kRowScale ? a.alpha * a.wscale[n] : a.alpha);
        if (a.bias) v[i] += (float)a.bias[n];
      }
      if constexpr (GLU) {
        // rows nb + 2 j (gate) and nb + 2 j + 1 (up) -> output column nb / 2 + j; N is even, so a pair is wholly
        // inside or outside N
        __bf16* c = a.C + m * a.ldc + (nb >> 1);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (nb + 2 * j < a.N) c[j] = (__bf16)(v[2 * j] / (1.f + __expf(-v[2 * j])) * v[2 * j + 1]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = apply_act(v[i], a.act);
          if (a.R && nb + i < a.N) v[i] += (float)a.R[m * a.ldr + nb + i];
        }
        __bf16* c = a.C + m * a.ldc + nb;
        if (a.vec && nb + 3 < a.N) {
          *reinterpret_cast<bf16x4*>(c) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (nb + i < a.N) c[i] = (__bf16)v[i];
        }
      }
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// TILES with tiles = 0, from the table in the header comment: 4 from N = 16384 (the LM head, the gated fc1), below
// that 2 from N = 4096 and 1 for narrower N (N = 2048 is 128 workgroups at TILES = 1 and loses at 2). MXFP4 takes 2 at
// narrow N as well, where its TILES = 1 form is the slowest of the three (a scale byte load per 16-B piece and four
// fragments per piece against one tile), except on a long K (measured: 2048 x 8192), where 64 workgroups are too few.
inline int choose_tiles(bool mx4, int N, int K) {
  if (N >= 16384) return 4;
  if (mx4) return N < 4096 && K > 4096 ? 1 : 2;
  return N >= 4096 ? 2 : 1;
}

template <class F, int MB, bool GLU>
void launch_tiles(const StreamArgs& a, int tiles, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 16 * tiles - 1) / (16 * tiles))), block(256);
  if (tiles == 4) hipLaunchKernelGGL((stream_wide<F, MB, 4, GLU>), grid, block, 0, s, a);
  else if (tiles == 2) hipLaunchKernelGGL((stream_wide<F, MB, 2, GLU>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((stream_wide<F, MB, 1, GLU>), grid, block, 0, s, a);
}

// ldw in BYTES here; kq: the format's K grid (8 / 16 / 32 = elements per 16-B piece)
template <class F, bool GLU>
int stream_launch(int tiles, const void* A, const void* W, const void* S, const float* wscale, void* C,
                  const void* bias, const void* R, int M, int N, int K, long long lda, long long ldw, long long lds,
                  long long ldc, long long ldr, float alpha, int act, void* stream) {
  constexpr int kq = 8 * F::NF;
  if (!A || !W || !C || (F::kGroupScale && !S) || (F::kRowScale && !wscale)) return KFAMD_EINVAL;
  if (M < 1 || M > kMaxM || N < 1 || K < kq || K % kq) return KFAMD_EINVAL;
  if (GLU) {
    if ((N & 1) || ldc < N / 2) return KFAMD_EINVAL;
  } else {
    if (act < KFAMD_ACT_NONE || act > KFAMD_ACT_SILU || (R && act != KFAMD_ACT_NONE)) return KFAMD_EINVAL;
    if (ldc < N || (R && ldr < N)) return KFAMD_EINVAL;
  }
  if (lda < K || ldw < (long long)K * 16 / kq || (F::kGroupScale && lds < K / 32)) return KFAMD_EINVAL;
  if (tiles != 0 && tiles != 1 && tiles != 2 && tiles != 4) return KFAMD_EINVAL;
  if (!al16(A) || !al16(W) || (lda & 7) || (ldw & 15)) return KFAMD_EALIGN;
  StreamArgs a;
  a.A = static_cast<const __bf16*>(A);
  a.W = static_cast<const uint8_t*>(W);
  a.S = static_cast<const uint8_t*>(S);
  a.wscale = wscale;
  a.C = static_cast<__bf16*>(C);
  a.bias = static_cast<const __bf16*>(bias);
  a.R = static_cast<const __bf16*>(R);
  a.M = M, a.N = N, a.K = K;
  a.lda = lda, a.ldw = ldw, a.lds = lds, a.ldc = ldc, a.ldr = ldr;
  a.alpha = alpha;
  a.act = act;
  a.vec = (reinterpret_cast<uintptr_t>(C) & 7) == 0 && (ldc & 3) == 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int t = tiles ? tiles : choose_tiles(F::kGroupScale, N, K);
  if (M <= 32) launch_tiles<F, 2, GLU>(a, t, s);
  else if (M <= 64) launch_tiles<F, 4, GLU>(a, t, s);
  else launch_tiles<F, 8, GLU>(a, t, s);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

// tiles: 0 = by (M, N) (choose_tiles), else the 16-row weight tiles per workgroup, 1 / 2 / 4
extern "C" int kfamd_gemm_nt_stream_bf16(int tiles, const void* A, const void* W, void* C, const void* bias,
                                         const void* R, int M, int N, int K, long long lda, long long ldw,
                                         long long ldc, long long ldr, float alpha, int act, void* stream) {
  return stream_launch<Bf16Weight, false>(tiles, A, W, nullptr, nullptr, C, bias, R, M, N, K, lda, ldw * 2, 0, ldc, ldr,
                                          alpha, act, stream);
}

extern "C" int kfamd_gemm_nt_stream_w8(int tiles, const void* A, const void* codes, const float* wscale, void* C,
                                       const void* bias, const void* R, int M, int N, int K, long long lda,
                                       long long ldw, long long ldc, long long ldr, float alpha, int act,
                                       void* stream) {
  return stream_launch<Fp8Weight, false>(tiles, A, codes, nullptr, wscale, C, bias, R, M, N, K, lda, ldw, 0, ldc, ldr,
                                         alpha, act, stream);
}

extern "C" int kfamd_gemm_nt_stream_mx4(int tiles, const void* A, const void* codes, const void* scales, void* C,
                                        const void* bias, const void* R, int M, int N, int K, long long lda,
                                        long long ldw_bytes, long long lds, long long ldc, long long ldr, float alpha,
                                        int act, void* stream) {
  return stream_launch<Mx4Weight, false>(tiles, A, codes, scales, nullptr, C, bias, R, M, N, K, lda, ldw_bytes, lds,
                                         ldc, ldr, alpha, act, stream);
}

// ---- gated (SwiGLU) entry points: W [N = 2F][K] interleaved (row 2j gate, 2j + 1 up), C [M][F] -----------------
extern "C" int kfamd_gemm_nt_stream_bf16_glu(int tiles, const void* A, const void* W, void* C, const void* bias, int M,
                                             int N, int K, long long lda, long long ldw, long long ldc, float alpha,
                                             void* stream) {
  return stream_launch<Bf16Weight, true>(tiles, A, W, nullptr, nullptr, C, bias, nullptr, M, N, K, lda, ldw * 2, 0, ldc,
                                         0, alpha, KFAMD_ACT_NONE, stream);
}

extern "C" int kfamd_gemm_nt_stream_w8_glu(int tiles, const void* A, const void* codes, const float* wscale, void* C,
                                           const void* bias, int M, int N, int K, long long lda, long long ldw,
                                           long long ldc, float alpha, void* stream) {
  return stream_launch<Fp8Weight, true>(tiles, A, codes, nullptr, wscale, C, bias, nullptr, M, N, K, lda, ldw, 0, ldc,
                                        0, alpha, KFAMD_ACT_NONE, stream);
}

extern "C" int kfamd_gemm_nt_stream_mx4_glu(int tiles, const void* A, const void* codes, const void* scales, void* C,
                                            const void* bias, int M, int N, int K, long long lda, long long ldw_bytes,
                                            long long lds, long long ldc, float alpha, void* stream) {
  return stream_launch<Mx4Weight, true>(tiles, A, codes, scales, nullptr, C, bias, nullptr, M, N, K, lda, ldw_bytes,
                                        lds, ldc, 0, alpha, KFAMD_ACT_NONE, stream);
}
