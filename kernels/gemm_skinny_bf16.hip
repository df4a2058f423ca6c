// gemm_skinny_bf16.hip — weight-streaming NT GEMM for decode: C[M][N] = act(alpha * A[M][K] . W[N][K]^T
// + bias[N]) (+ R[M][N]) with 1 <= M <= 16.
//
// With M = batch the 128x128 tile kernels spend >= 7/8 of every tile on padding; the operation is a
// single pass over W (N * K * 2 bytes) against an L2-resident A (<= 16 x K). So W is read exactly
// once from HBM, straight to VGPRs in 16-B pieces with no LDS round trip (cdna_hip_programming.md §5,
// row "GEMV / M <= 16 decode weights"), the loads of several K chunks issued back to back before the
// first is consumed. fp32 accumulation, no atomics: the result is deterministic.
//
// Two arithmetic patterns behind one launcher:
//   VALU (skinny_valu<MR, ROWS>): a wave owns ROWS weight rows over the whole K; lane l takes the
//     16-B pieces l, l + 64, ... of every row, multiplies with the MR activation rows' matching
//     pieces and the ROWS * MR sums meet in wave_sum (wave_ops.h). 8 * MR FMAs per 16 weight bytes.
//   MFMA (skinny_mfma<TILES>): a 256-thread workgroup owns TILES x 8 weight rows and splits K over its
//     4 waves in 64-element chunks. Per chunk a wave loads 8 rows x 128 B (full lines: lane l = row
//     l & 7, piece l >> 3) and feeds them to v_mfma_f32_16x16x32_bf16 as the 16-row operand: operand
//     row r holds weight row r & 7 at k-piece 2q + (r >> 3) (q = lane >> 4), i.e. rows 0-7 carry the
//     even pieces and rows 8-15 the odd pieces of the SAME weight rows. Two MFMAs per chunk, one with
//     the activations' even pieces and one with their odd pieces as the 16-column operand (activation
//     rows zero-extended to 16 by clamping: a column only depends on its own activation row); result
//     rows 0-7 of the first plus rows 8-15 of the second are the chunk's product. The waves' partials
//     meet in LDS and are summed in a fixed order; 128 threads run the epilogue.
//   An 8-row tile keeps N = 2048 (gpt-1b d_model) at 256 workgroups, one per CU; wider N takes
//   TILES = 2 / 4 so the activation fragments (re-read from L2 per tile) are shared.
//
// Cut-over: kfamd_gemm_nt_skinny_bf16 runs the VALU form at M = 1 (kValuMaxM) below N = kValuMaxN and the
// MFMA form everywhere else; kfamd_gemm_nt_skinny_bf16_path forces either form. Measured on the gpt-1b
// shapes with both forms forced at M = 1, 2, 4, 8 (tools/decode_bench.py, profiles/decode/README.md; us per
// call VALU / MFMA): M = 1: 10.5 / 14.5 at 2048x8192, 11.5 / 12.4 at 8192x2048, level at 6144x2048 and
// 2048x2048, 32.4 / 29.7 at 32000x2048; M = 2: level (within the run's 5 % spread) except 35.4 / 29.7 at
// 32000x2048; M = 4: 15.3 / 12.5, 16.9 / 14.9, 41.4 / 29.7; M = 8: 20.7 / 12.4, 19.5 / 15.5, 62.9 / 29.8.
// The MFMA form's time hardly depends on M, the VALU form's FMA count grows with it. The VALU
// instantiations for 2..8 activation rows are therefore reached only through the forced path: they are
// kept so that this measurement can be repeated, not for production use.
//
// Gated form (GLU template parameter, kfamd_gemm_nt_skinny_bf16_glu*): the same kernels with a SwiGLU epilogue
// over interleaved (gate, up) weight rows, see glu_store. Its cut-overs are its own, from tools/decode_bench.py
// --steps glu (profiles/glu/README.md; K = 2048, medians of 7 interleaved blocks, us per call from Python,
// weights rotated past the last-level cache), N = 2F at F = 5504 / 8192:
//   M = 1: VALU at 2 rows (one pair) per wave 12.5 / 14.6, at 4 rows 14.4 / 19.2; MFMA TILES 1 / 2 / 4: 13.3 /
//     15.4 / 14.8 and 16.5 / 19.6 / 17.9. Hence M = 1 takes the VALU form at 2 rows per wave at every N up to
//     16384 (kGluValuMaxN: nothing wider was measured), where the ungated kernel takes 4 rows from N = 8192.
//   M = 2: VALU 2 rows 14.1 / 16.8 against MFMA TILES 1 13.8 / 16.9: level, MFMA keeps it. M = 4: VALU 15.8 /
//     20.3, MFMA TILES 1 / 2 / 4 14.6 / 15.5 / 15.0 and 18.1 / 19.4 / 17.8. M = 8: 16.3 / 15.8 / 15.3 and 21.0 /
//     20.2 / 17.8. M = 16: 20.1 / 17.1 / 15.3 and 25.9 / 22.7 / 17.9.
//   Hence from N = 8192 (kGluWideN) the MFMA form runs TILES = 1 at M <= 4 and TILES = 4 above (the ungated
//   thresholds would give 2 at N = 11008: 17.1 against 15.3 at M = 16); narrower N was not measured and keeps the
//   ungated thresholds. The two-launch form (this GEMM ungated to [M, 2F], then swiglu_bf16.hip) took 19.4 - 20.9 us
//   at every one of these points: the gated launch (13.0 - 18.2) wins at each, by 2 to 7 us.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kValuMaxM = 1;
// the gated form's own cut-overs (the GLU table in the header comment)
constexpr int kGluValuMaxM = 1;
constexpr int kGluValuMaxN = 16384;  // inclusive: 2 x 8192, the widest gated shape measured
constexpr int kGluWideN = 8192;      // from here the MFMA tile count follows M, below it the ungated thresholds
constexpr int kValuMaxN = 16384;  // the 32000-row LM head streams faster on the MFMA form even at M = 1

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

__device__ __forceinline__ void unpack8(const u32x4& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

struct SkinnyArgs {
  const __bf16* A;
  const __bf16* W;
  __bf16* C;
  const __bf16* bias;
  const __bf16* R;
  int M, N, K;
  long long lda, ldw, ldc, ldr;
  float alpha;
  int act;
};

__device__ __forceinline__ void epilogue_store(const SkinnyArgs& a, int m, int n, float acc) {
  float v = acc * a.alpha;
  if (a.bias) v += (float)a.bias[n];
  v = apply_act(v, a.act);
  if (a.R) v += (float)a.R[m * a.ldr + n];
  a.C[m * a.ldc + n] = (__bf16)v;
}

// GLU (the gated form, kfamd_gemm_nt_skinny_bf16_glu*): weight rows n (even) and n + 1 are gate and up of output
// column n / 2 (ops/swiglu.py states the rule): C[m][n / 2] = silu(z[n]) * z[n + 1], z = alpha * acc + bias, all
// in fp32, rounded once. No activation code, no residual; a.N is the weight's row count 2F.
__device__ __forceinline__ void glu_store(const SkinnyArgs& a, int m, int n, float accg, float accu) {
  float g = accg * a.alpha, u = accu * a.alpha;
  if (a.bias) {
    g += (float)a.bias[n];
    u += (float)a.bias[n + 1];
  }
  a.C[m * a.ldc + (n >> 1)] = (__bf16)(g / (1.f + __expf(-g)) * u);
}

// ---- VALU form -------------------------------------------------------------------------------
template <int MR, int ROWS, bool GLU = false>
__global__ __launch_bounds__(256) void skinny_valu(SkinnyArgs a) {
  constexpr int U = 2;  // 16-B pieces per row in flight per lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= a.N) return;  // wave-uniform; no barrier in this kernel
  const int pieces = a.K / 8;
  float acc[ROWS][MR];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;
  const __bf16* wrow[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wrow[r] = a.W + (long long)min(n0 + r, a.N - 1) * a.ldw;
  const __bf16* arow[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) arow[m] = a.A + (long long)min(m, a.M - 1) * a.lda;

  for (int p0 = 0; p0 < pieces; p0 += 64 * U) {
    u32x4 w[U][ROWS], x[U][MR];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * 64 + lane;
      ok[u] = p < pieces;
      const int pc = ok[u] ? p : 0;  // a clamped (valid) address; its products are not accumulated
#pragma unroll
      for (int r = 0; r < ROWS; ++r) w[u][r] = *reinterpret_cast<const u32x4*>(wrow[r] + pc * 8);
#pragma unroll
      for (int m = 0; m < MR; ++m) x[u][m] = *reinterpret_cast<const u32x4*>(arow[m] + pc * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
      float xf[MR][8];
#pragma unroll
      for (int m = 0; m < MR; ++m) unpack8(x[u][m], xf[m]);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        float wf[8];
        unpack8(w[u][r], wf);
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[r][m] = fmaf(wf[i], xf[m][i], acc[r][m]);
      }
    }
  }
  if constexpr (GLU) {
    // ROWS is even and so is n0: the wave's rows are ROWS / 2 whole (gate, up) pairs; N is even, so a pair
    // is wholly inside or wholly outside N
#pragma unroll
    for (int r = 0; r < ROWS; r += 2)
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const float sg = kfw::wave_sum(acc[r][m]), su = kfw::wave_sum(acc[r + 1][m]);
        if (lane == 0 && n0 + r < a.N && m < a.M) glu_store(a, m, n0 + r, sg, su);
      }
  } else {
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const float s = kfw::wave_sum(acc[r][m]);
        if (lane == 0 && n0 + r < a.N && m < a.M) epilogue_store(a, m, n0 + r, s);
      }
  }
}

// ---- MFMA form -------------------------------------------------------------------------------
template <int TILES, bool GLU = false>
__global__ __launch_bounds__(256) void skinny_mfma(SkinnyArgs a) {
  constexpr int U = 4;  // K chunks (64 elements) in flight per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * (8 * TILES);
  const int nchunks = (a.K + 63) / 64;
  // W fragment: row lane & 7 of each tile, 16-B piece lane >> 3 of the chunk
  const int wpiece = lane >> 3;
  const __bf16* wrow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) wrow[t] = a.W + (long long)min(n0 + t * 8 + (lane & 7), a.N - 1) * a.ldw;
  // activation fragments: row lane & 15 (clamped), pieces 2q and 2q + 1 (32 contiguous bytes)
  const int q = lane >> 4;
  const __bf16* arow = a.A + (long long)min(lane & 15, a.M - 1) * a.lda;

  f32x4 acc_e[TILES], acc_o[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc_e[t] = acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};

  for (int c0 = wave; c0 < nchunks; c0 += 4 * U) {
    u32x4 w[U][TILES], xe[U], xo[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u * 4;
      const int kw = c * 64 + wpiece * 8, ke = c * 64 + q * 16, ko = ke + 8;
      const bool live = c < nchunks;  // wave-uniform
      // K % 8 == 0: a piece lies wholly inside or wholly outside K; outside pieces are zero in BOTH
      // operands (the address is clamped to piece 0 of the row)
      const bool wok = live && kw < a.K, eok = live && ke < a.K, ook = live && ko < a.K;
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(wrow[t] + (wok ? kw : 0));
        w[u][t] = wok ? v : zero;
      }
      const u32x4 ve = *reinterpret_cast<const u32x4*>(arow + (eok ? ke : 0));
      const u32x4 vo = *reinterpret_cast<const u32x4*>(arow + (ook ? ko : 0));
      xe[u] = eok ? ve : zero;
      xo[u] = ook ? vo : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16x8 be = __builtin_bit_cast(bf16x8, xe[u]), bo = __builtin_bit_cast(bf16x8, xo[u]);
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const bf16x8 wf = __builtin_bit_cast(bf16x8, w[u][t]);
        acc_e[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, be, acc_e[t], 0, 0, 0);
        acc_o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, bo, acc_o[t], 0, 0, 0);
      }
    }
  }

  // result layout: lane holds column (activation row) lane & 15, operand rows 4q + i. Rows 0-7 of the
  // even product and rows 8-15 of the odd product belong to weight row (4q + i) & 7.
  __shared__ float red[4][2][TILES][8][16];
  const int m = lane & 15;
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * q + i;
      red[wave][row >> 3][t][row & 7][m] = (row < 8) ? acc_e[t][i] : acc_o[t][i];
    }
  __syncthreads();
  if constexpr (GLU) {
    // an 8-row tile is 4 (gate, up) pairs: a thread sums the waves' partials of both rows of one pair, in the
    // ungated epilogue's order, then gates
    for (int e = threadIdx.x; e < TILES * 64; e += 256) {
      const int pr = e & 3, mm = (e >> 2) & 15, t = e >> 6;
      const int n = n0 + t * 8 + 2 * pr;
      if (mm >= a.M || n >= a.N) continue;
      float sg = 0.f, su = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        sg += red[wv][0][t][2 * pr][mm] + red[wv][1][t][2 * pr][mm];
        su += red[wv][0][t][2 * pr + 1][mm] + red[wv][1][t][2 * pr + 1][mm];
      }
      glu_store(a, mm, n, sg, su);
    }
  } else {
    for (int e = threadIdx.x; e < TILES * 128; e += 256) {
      const int wr = e & 7, mm = (e >> 3) & 15, t = e >> 7;
      const int n = n0 + t * 8 + wr;
      if (mm >= a.M || n >= a.N) continue;
      float s = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) s += red[wv][0][t][wr][mm] + red[wv][1][t][wr][mm];
      epilogue_store(a, mm, n, s);
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int ROWS, bool GLU>
void launch_valu(const SkinnyArgs& a, int mr, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 4 * ROWS - 1) / (4 * ROWS))), block(256);
  switch (mr) {
    case 1: hipLaunchKernelGGL((skinny_valu<1, ROWS, GLU>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((skinny_valu<2, ROWS, GLU>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((skinny_valu<4, ROWS, GLU>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((skinny_valu<8, ROWS, GLU>), grid, block, 0, s, a); break;
  }
}

template <int TILES, bool GLU>
void launch_mfma(const SkinnyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((skinny_mfma<TILES, GLU>), dim3((unsigned)((a.N + 8 * TILES - 1) / (8 * TILES))), dim3(256), 0, s,
                     a);
}

// tiles: 0 = by N; else the MFMA form's TILES (1, 2, 4) or the VALU form's weight rows per wave (2, 4; 8 activation
// rows always take 2). The ungated entry points pass 0.
template <bool GLU>
int skinny_launch(int path, int tiles, const void* A, const void* W, void* C, const void* bias, const void* R, int M,
                  int N, int K, long long lda, long long ldw, long long ldc, long long ldr, float alpha, int act,
                  void* stream) {
  if (!A || !W || !C || M < 1 || M > 16 || N < 1 || K < 8 || K % 8) return KFAMD_EINVAL;
  if (GLU) {
    if ((N & 1) || ldc < N / 2) return KFAMD_EINVAL;
  } else {
    if (act < KFAMD_ACT_NONE || act > KFAMD_ACT_SILU || (R && act != KFAMD_ACT_NONE)) return KFAMD_EINVAL;
    if (ldc < N || (R && ldr < N)) return KFAMD_EINVAL;
  }
  if (lda < K || ldw < K) return KFAMD_EINVAL;
  if (path < 0 || path > 2 || (path == 1 && M > 8)) return KFAMD_EINVAL;
  const bool valu = path == 1 || (path == 0 && (GLU ? M <= kGluValuMaxM && N <= kGluValuMaxN
                                                     : M <= kValuMaxM && N < kValuMaxN));
  if (tiles != 0 && (valu ? (tiles != 2 && tiles != 4) : (tiles != 1 && tiles != 2 && tiles != 4))) return KFAMD_EINVAL;
  if (!al16(A) || !al16(W) || (lda & 7) || (ldw & 7)) return KFAMD_EALIGN;
  SkinnyArgs a;
  a.A = static_cast<const __bf16*>(A);
  a.W = static_cast<const __bf16*>(W);
  a.C = static_cast<__bf16*>(C);
  a.bias = static_cast<const __bf16*>(bias);
  a.R = static_cast<const __bf16*>(R);
  a.M = M, a.N = N, a.K = K;
  a.lda = lda, a.ldw = ldw, a.ldc = ldc, a.ldr = ldr;
  a.alpha = alpha;
  a.act = act;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (valu) {
    const int mr = M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8));
    // weight rows per wave: 2 keeps N = 2048 at 256 workgroups; 4 shares the activation pieces wider
    // (gated: 2 at every N, one pair per wave: 4 rows lost at every measured M and N)
    const int rows = mr > 4 ? 2 : (tiles ? tiles : (N >= 8192 && !GLU ? 4 : 2));
    if (rows == 4) launch_valu<4, GLU>(a, mr, s);
    else launch_valu<2, GLU>(a, mr, s);
  } else {
    const int t = tiles ? tiles
                        : (GLU && N >= kGluWideN ? (M <= 4 ? 1 : 4) : (N >= 16384 ? 4 : (N >= 4096 ? 2 : 1)));
    if (t == 4) launch_mfma<4, GLU>(a, s);
    else if (t == 2) launch_mfma<2, GLU>(a, s);
    else launch_mfma<1, GLU>(a, s);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

// path: 0 = by M (kValuMaxM), 1 = VALU (M <= 8), 2 = MFMA
extern "C" int kfamd_gemm_nt_skinny_bf16_path(int path, const void* A, const void* W, void* C, const void* bias,
                                              const void* R, int M, int N, int K, long long lda, long long ldw,
                                              long long ldc, long long ldr, float alpha, int act, void* stream) {
  return skinny_launch<false>(path, 0, A, W, C, bias, R, M, N, K, lda, ldw, ldc, ldr, alpha, act, stream);
}

extern "C" int kfamd_gemm_nt_skinny_bf16(const void* A, const void* W, void* C, const void* bias, const void* R, int M,
                                         int N, int K, long long lda, long long ldw, long long ldc, long long ldr,
                                         float alpha, int act, void* stream) {
  return kfamd_gemm_nt_skinny_bf16_path(0, A, W, C, bias, R, M, N, K, lda, ldw, ldc, ldr, alpha, act, stream);
}

// ---- gated (SwiGLU) entry points: W [N = 2F][K] interleaved (row 2j gate, 2j + 1 up), C [M][F] ----------------
extern "C" int kfamd_gemm_nt_skinny_bf16_glu_tiles(int path, int tiles, const void* A, const void* W, void* C,
                                                   const void* bias, int M, int N, int K, long long lda, long long ldw,
                                                   long long ldc, float alpha, void* stream) {
  return skinny_launch<true>(path, tiles, A, W, C, bias, nullptr, M, N, K, lda, ldw, ldc, 0, alpha, KFAMD_ACT_NONE,
                             stream);
}

extern "C" int kfamd_gemm_nt_skinny_bf16_glu_path(int path, const void* A, const void* W, void* C, const void* bias,
                                                  int M, int N, int K, long long lda, long long ldw, long long ldc,
                                                  float alpha, void* stream) {
  return kfamd_gemm_nt_skinny_bf16_glu_tiles(path, 0, A, W, C, bias, M, N, K, lda, ldw, ldc, alpha, stream);
}

extern "C" int kfamd_gemm_nt_skinny_bf16_glu(const void* A, const void* W, void* C, const void* bias, int M, int N,
                                             int K, long long lda, long long ldw, long long ldc, float alpha,
                                             void* stream) {
  return kfamd_gemm_nt_skinny_bf16_glu_tiles(0, 0, A, W, C, bias, M, N, K, lda, ldw, ldc, alpha, stream);
}
