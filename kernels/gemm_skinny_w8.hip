// gemm_skinny_w8.hip — weight-streaming NT GEMM on 8-bit weights (W8A16) for decode:
//   C[M][N] = act(alpha * wscale[n] * (A[M][K] . codes[N][K]^T) + bias[n]) (+ R[M][N]),  1 <= M <= 16.
// A, bias, R, C are bf16; codes are OCP e4m3fn bytes (row stride ldw bytes) with one fp32 scale per
// output row (ops.decode.quantize_rows: the FP8 KV cache's format). Activations stay bf16, accumulation
// fp32. Every e4m3fn value is a bf16 value, so the products are exact as in gemm_skinny_bf16.hip and the
// row scale is applied once, in fp32, in the epilogue (before bias, activation and residual; the bias is
// not scaled). NaN codes (0x7F, 0xFF) are out of contract.
//
// The design is gemm_skinny_bf16.hip's (cdna_hip_programming.md §5, row "GEMV / M <= 16 decode
// weights"): the codes are read exactly once from HBM in 16-B loads straight to VGPRs, no LDS staging,
// the loads of several K chunks issued before the first is consumed, a fixed summation order and no
// atomics (deterministic). Codes are widened in registers (v_cvt_pk_f32_fp8, then the upper halves of two
// fp32 packed into a bf16 pair by v_perm_b32: exact); nothing dequantised is written to memory. A 16-B
// piece now holds 16 k-elements, which changes the geometry of both forms:
//   VALU (skinny_w8_valu<MR, ROWS>): a wave owns ROWS weight rows over the whole K; lane l takes the 16-B
//     pieces l, l + 64, ... of every row (8 lanes per 128-B line) and the matching 32 B of the MR
//     activation rows; codes -> fp32, 16 * MR FMAs per piece, the ROWS * MR sums meet in wave_sum.
//   MFMA (skinny_w8_mfma<TILES>): a 256-thread workgroup owns TILES x 8 weight rows and splits K over its
//     4 waves in 128-element chunks. Per chunk a wave loads 8 rows x 128 B (full lines: lane l = row
//     l & 7, piece l >> 3) and widens each piece into two bf16x8 (codes 0-7 / 8-15). As the 16-row operand
//     of v_mfma_f32_16x16x32_bf16, operand row r then holds weight row r & 7 at k = 32q + 16 (r >> 3)
//     (+ 8 for the upper half), q = lane >> 4: the four 8-element activation pieces a lane needs are the
//     32 contiguous elements 32q .. 32q + 31 of its activation row. Four MFMAs per chunk: lower half x
//     pieces 0 / 2, upper half x pieces 1 / 3; pieces 0, 1 accumulate into acc_e (rows 0-7 valid), 2, 3
//     into acc_o (rows 8-15 valid). Reduction over the waves and epilogue as in the bf16 kernel. The
//     fp8 x fp8 MFMA is not used: it would need quantised activations.
//
// Cut-over (kfamd_gemm_nt_skinny_w8, path 0): the VALU form at M <= 2 (kValuMaxM) below N = kValuMaxN, the
// MFMA form everywhere else; kfamd_gemm_nt_skinny_w8_path forces either form. Measured on the gpt-1b shapes
// with both forms and every tile count forced at M = 1, 2, 4, 8, 16 (tools/decode_bench.py --steps w8,
// profiles/w8/README.md; medians of 7 interleaved blocks, us per call from Python, so ~10.3 us is the launch
// floor and most N x 2048 shapes sit on it in both forms). What separates, VALU / MFMA:
//   2048x8192: M = 1 10.5 / 13.1, M = 2 10.7 / 13.4, M = 4 11.0 / 13.9, M = 8 24.1 / 14.4 (supposed, not
//     profiled: with TILES = 1 every 8-row tile re-reads 64 activation bytes per 16 weight bytes from L2,
//     twice the bf16 kernel's share); the VALU form's FMA count passes the MFMA form between M = 4 and 8;
//   8192x2048: M = 4 11.7 / 10.6, M = 8 16.9 / 10.6; 6144x2048: M = 8 15.4 / 10.7;
//   32000x2048 (4 weight rows per wave / TILES = 4): M = 1 18.3 / 16.7, M = 2 21.0 / 16.4, M = 4 33.9 / 16.6,
//     M = 8 60.3 / 18.2.
// So M <= 2 takes the VALU form (a win at 2048x8192, level elsewhere below N = 16384), M = 4 does not (it
// would lose at 8192x2048), and the LM head stays on the MFMA form at every M. The VALU instantiations for 4
// and 8 activation rows are reached through the forced path only: kept so that this can be measured again.
// Tile counts by N, forced at every M (us at TILES 1 / 2 / 4): 32000x2048 M = 1 25.3 / 20.9 / 16.7, M = 16
// 45.0 / 31.7 / 21.6; 8192x2048 M = 16 13.4 / 10.6 / 10.6, level at M <= 8; 6144x2048 and 2048x2048 level;
// 2048x8192 M = 1 13.1 / 15.7 / 22.5 (too few workgroups). Hence TILES = 1 below N = 4096, 2 below 16384, 4
// from there, the bf16 kernel's thresholds. VALU weight rows per wave: 2 below N = 8192, 4 from there (M <= 4):
// 8192x2048 M = 4 12.6 / 11.6 at 2 / 4 rows, 2048x8192 M = 2 10.6 / 13.4.
//
// Gated form (GLU template parameter, kfamd_gemm_nt_skinny_w8_glu*): the same kernels with a SwiGLU epilogue over
// interleaved (gate, up) rows, see glu_store. Measured with tools/decode_bench.py --steps glu
// (profiles/glu/README.md; K = 2048, N = 2F at F = 5504 / 8192, medians of 7 interleaved blocks, us per call from
// Python): every form and tile count sits on the launch floor, 11.7 - 12.5 us, at M <= 2 (MFMA TILES = 1 at F =
// 8192 13.0 - 13.5); the VALU form leaves it at M = 4 for F = 8192 (16.4 against MFMA 12.5) and at M = 8 (23.7 /
// 29.8 against 12.0 / 12.5); MFMA TILES = 1 loses from M = 8 (13.2 / 16.4) and TILES = 2 at M = 16 (13.7 / 17.4
// against TILES = 4 11.8 / 12.3). So the gated form keeps the ungated cut-overs (kGluValuMaxM = kValuMaxM, the same
// thresholds on N) with one exception: the ungated thresholds give N = 11008 TILES = 2, which at M = 16 is that
// 13.7 (13.6 - 13.8) against 11.8 (11.7 - 11.9), so from N = 8192 (kGluWideN) more than 8 activation rows take
// TILES = 4 (level at M = 8: 11.9 / 11.8). The two-launch form (the ungated GEMM to [M, 2F], then swiglu_bf16.hip)
// took 18.3 - 19.5 us at every point: the gated launch (11.7 - 12.7) wins each by about 7 us.
//
// Registers (gfx950 compile, -Rpass-analysis=kernel-resource-usage; 0 scratch bytes in every
// instantiation; VGPRs / AGPRs): skinny_w8_mfma<1> 90 / 8, <2> 107 / 24, <4> 77 / 44 (U = 2);
// skinny_w8_valu<MR, ROWS>: <1,2> 72 / 0, <2,2> 92 / 0, <4,2> 130 / 0, <8,2> 120 / 0 (U = 1), <1,4> 138 / 0,
// <2,4> 126 / 0, <4,4> 164 / 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kValuMaxM = 2;
// the gated form's own cut-overs (the GLU paragraph of the header comment)
constexpr int kGluValuMaxM = 2;
constexpr int kGluWideN = 8192;  // from here more than 8 activation rows take TILES = 4 (ungated: from N = 16384)
constexpr int kValuMaxN = 16384;  // the 32000-row LM head streams faster on the MFMA form at every M

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

// 8 bf16 (one 16-B piece of an activation row) -> fp32
__device__ __forceinline__ void unpack8(const u32x4& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

// 4 e4m3 codes (memory order: byte 0 first) -> fp32
__device__ __forceinline__ void codes4(unsigned w, float* f) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0], f[1] = lo[1], f[2] = hi[0], f[3] = hi[1];
}

// 8 e4m3 codes (two dwords) -> 8 bf16, exact: the upper 16 bits of each fp32 (its lower 16 are zero)
__device__ __forceinline__ bf16x8 codes8_bf16(unsigned w0, unsigned w1) {
  float f[8];
  codes4(w0, f);
  codes4(w1, f + 4);
  u32x4 p;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    p[i] = __builtin_amdgcn_perm(__float_as_uint(f[2 * i + 1]), __float_as_uint(f[2 * i]), 0x07060302u);
  return __builtin_bit_cast(bf16x8, p);
}

struct W8Args {
  const __bf16* A;
  const uint8_t* W;      // e4m3fn codes [N][ldw]
  const float* wscale;   // [N]
  __bf16* C;
  const __bf16* bias;
  const __bf16* R;
  int M, N, K;
  long long lda, ldw, ldc, ldr;
  float alpha;
  int act;
};

__device__ __forceinline__ void epilogue_store(const W8Args& a, int m, int n, float acc) {
  float v = acc * (a.alpha * a.wscale[n]);
  if (a.bias) v += (float)a.bias[n];
  v = apply_act(v, a.act);
  if (a.R) v += (float)a.R[m * a.ldr + n];
  a.C[m * a.ldc + n] = (__bf16)v;
}

// GLU (the gated form, kfamd_gemm_nt_skinny_w8_glu*): as in gemm_skinny_bf16.hip, weight rows n (even) and n + 1
// are gate and up of output column n / 2; each row's scale is applied before its bias, as in the ungated epilogue.
__device__ __forceinline__ void glu_store(const W8Args& a, int m, int n, float accg, float accu) {
  float g = accg * (a.alpha * a.wscale[n]), u = accu * (a.alpha * a.wscale[n + 1]);
  if (a.bias) {
    g += (float)a.bias[n];
    u += (float)a.bias[n + 1];
  }
  a.C[m * a.ldc + (n >> 1)] = (__bf16)(g / (1.f + __expf(-g)) * u);
}

// ---- VALU form -------------------------------------------------------------------------------
template <int MR, int ROWS, bool GLU = false>
__global__ __launch_bounds__(256) void skinny_w8_valu(W8Args a) {
  constexpr int U = MR >= 8 ? 1 : 2;  // 16-B pieces per row in flight per lane (16 * MR activation bytes each)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= a.N) return;  // wave-uniform; no barrier in this kernel
  const int pieces = a.K / 16;
  float acc[ROWS][MR];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;
  const uint8_t* wrow[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wrow[r] = a.W + (long long)min(n0 + r, a.N - 1) * a.ldw;
  const __bf16* arow[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) arow[m] = a.A + (long long)min(m, a.M - 1) * a.lda;

  for (int p0 = 0; p0 < pieces; p0 += 64 * U) {
    u32x4 w[U][ROWS], x[U][MR][2];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * 64 + lane;
      ok[u] = p < pieces;
      const int pc = ok[u] ? p : 0;  // a clamped (valid) address; its products are not accumulated
#pragma unroll
      for (int r = 0; r < ROWS; ++r) w[u][r] = *reinterpret_cast<const u32x4*>(wrow[r] + pc * 16);
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int h = 0; h < 2; ++h) x[u][m][h] = *reinterpret_cast<const u32x4*>(arow[m] + pc * 16 + h * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // the piece's codes 0-7, then 8-15
        float xf[MR][8];
#pragma unroll
        for (int m = 0; m < MR; ++m) unpack8(x[u][m][h], xf[m]);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float wf[8];
          codes4(w[u][r][2 * h], wf);
          codes4(w[u][r][2 * h + 1], wf + 4);
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[r][m] = fmaf(wf[i], xf[m][i], acc[r][m]);
        }
      }
    }
  }
  if constexpr (GLU) {
    // ROWS and n0 are even: the wave's rows are ROWS / 2 whole (gate, up) pairs, and with N even a pair is
    // wholly inside or wholly outside N
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
__global__ __launch_bounds__(256) void skinny_w8_mfma(W8Args a) {
  constexpr int U = TILES >= 4 ? 2 : 4;  // K chunks (128 elements) in flight per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * (8 * TILES);
  const int nchunks = (a.K + 127) / 128;
  // W fragment: row lane & 7 of each tile, 16-B piece (16 codes) lane >> 3 of the chunk
  const int wpiece = lane >> 3;
  const uint8_t* wrow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) wrow[t] = a.W + (long long)min(n0 + t * 8 + (lane & 7), a.N - 1) * a.ldw;
  // activation fragments: row lane & 15 (clamped), elements 32q .. 32q + 31 of the chunk (64 contiguous bytes)
  const int q = lane >> 4;
  const __bf16* arow = a.A + (long long)min(lane & 15, a.M - 1) * a.lda;

  f32x4 acc_e[TILES], acc_o[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc_e[t] = acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};

  for (int c0 = wave; c0 < nchunks; c0 += 4 * U) {
    u32x4 w[U][TILES], x[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u * 4;
      const bool live = c < nchunks;  // wave-uniform
      // K % 16 == 0: a 16-code piece and each 8-element activation piece lie wholly inside or wholly
      // outside K; outside pieces are zero in BOTH operands (the address is clamped to the row's start)
      const int kw = c * 128 + wpiece * 16;
      const bool wok = live && kw < a.K;
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(wrow[t] + (wok ? kw : 0));
        w[u][t] = wok ? v : zero;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kx = c * 128 + q * 32 + i * 8;
        const bool xok = live && kx < a.K;
        const u32x4 v = *reinterpret_cast<const u32x4*>(arow + (xok ? kx : 0));
        x[u][i] = xok ? v : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bf16x8 b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = __builtin_bit_cast(bf16x8, x[u][i]);
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const bf16x8 lo = codes8_bf16(w[u][t][0], w[u][t][1]), hi = codes8_bf16(w[u][t][2], w[u][t][3]);
        acc_e[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, b[0], acc_e[t], 0, 0, 0);
        acc_e[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, b[1], acc_e[t], 0, 0, 0);
        acc_o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, b[2], acc_o[t], 0, 0, 0);
        acc_o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, b[3], acc_o[t], 0, 0, 0);
      }
    }
  }

  // result layout: lane holds column (activation row) lane & 15, operand rows 4q + i. Rows 0-7 of acc_e
  // and rows 8-15 of acc_o belong to weight row (4q + i) & 7.
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
void launch_valu(const W8Args& a, int mr, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 4 * ROWS - 1) / (4 * ROWS))), block(256);
  switch (mr) {
    case 1: hipLaunchKernelGGL((skinny_w8_valu<1, ROWS, GLU>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((skinny_w8_valu<2, ROWS, GLU>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((skinny_w8_valu<4, ROWS, GLU>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((skinny_w8_valu<8, 2, GLU>), dim3((unsigned)((a.N + 7) / 8)), block, 0, s, a); break;
  }
}

template <int TILES, bool GLU>
void launch_mfma(const W8Args& a, hipStream_t s) {
  hipLaunchKernelGGL((skinny_w8_mfma<TILES, GLU>), dim3((unsigned)((a.N + 8 * TILES - 1) / (8 * TILES))), dim3(256), 0,
                     s, a);
}

template <bool GLU>
int w8_launch(int path, int tiles, const void* A, const void* codes, const float* wscale, void* C, const void* bias,
              const void* R, int M, int N, int K, long long lda, long long ldw, long long ldc, long long ldr,
              float alpha, int act, void* stream) {
  if (!A || !codes || !wscale || !C || M < 1 || M > 16 || N < 1 || K < 16 || K % 16) return KFAMD_EINVAL;
  if (GLU) {
    if ((N & 1) || ldc < N / 2) return KFAMD_EINVAL;
  } else {
    if (act < KFAMD_ACT_NONE || act > KFAMD_ACT_SILU || (R && act != KFAMD_ACT_NONE)) return KFAMD_EINVAL;
    if (ldc < N || (R && ldr < N)) return KFAMD_EINVAL;
  }
  if (lda < K || ldw < K) return KFAMD_EINVAL;
  if (path < 0 || path > 2 || (path == 1 && M > 8)) return KFAMD_EINVAL;
  const bool valu = path == 1 || (path == 0 && M <= (GLU ? kGluValuMaxM : kValuMaxM) && N < kValuMaxN);
  if (tiles != 0 && (valu ? (tiles != 2 && tiles != 4) : (tiles != 1 && tiles != 2 && tiles != 4))) return KFAMD_EINVAL;
  if (!al16(A) || !al16(codes) || (lda & 7) || (ldw & 15)) return KFAMD_EALIGN;
  W8Args a;
  a.A = static_cast<const __bf16*>(A);
  a.W = static_cast<const uint8_t*>(codes);
  a.wscale = wscale;
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
    const int rows = tiles ? tiles : (N >= 8192 && mr <= 4 ? 4 : 2);
    if (rows == 4) launch_valu<4, GLU>(a, mr, s);
    else launch_valu<2, GLU>(a, mr, s);
  } else {
    const int t = tiles ? tiles : (N >= 16384 || (GLU && N >= kGluWideN && M > 8) ? 4 : (N >= 4096 ? 2 : 1));
    if (t == 4) launch_mfma<4, GLU>(a, s);
    else if (t == 2) launch_mfma<2, GLU>(a, s);
    else launch_mfma<1, GLU>(a, s);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

// path: 0 = by M and N (kValuMaxM, kValuMaxN), 1 = VALU (M <= 8), 2 = MFMA. tiles: 0 = by N; else the MFMA form's TILES
// (1, 2, 4) or the VALU form's weight rows per wave (2, 4; 8 activation rows always take 2).
extern "C" int kfamd_gemm_nt_skinny_w8_tiles(int path, int tiles, const void* A, const void* codes,
                                             const float* wscale, void* C, const void* bias, const void* R, int M,
                                             int N, int K, long long lda, long long ldw, long long ldc,
                                             long long ldr, float alpha, int act, void* stream) {
  return w8_launch<false>(path, tiles, A, codes, wscale, C, bias, R, M, N, K, lda, ldw, ldc, ldr, alpha, act, stream);
}

extern "C" int kfamd_gemm_nt_skinny_w8_path(int path, const void* A, const void* codes, const float* wscale, void* C,
                                            const void* bias, const void* R, int M, int N, int K, long long lda,
                                            long long ldw, long long ldc, long long ldr, float alpha, int act,
                                            void* stream) {
  return kfamd_gemm_nt_skinny_w8_tiles(path, 0, A, codes, wscale, C, bias, R, M, N, K, lda, ldw, ldc, ldr, alpha, act,
                                       stream);
}

extern "C" int kfamd_gemm_nt_skinny_w8(const void* A, const void* codes, const float* wscale, void* C, const void* bias,
                                       const void* R, int M, int N, int K, long long lda, long long ldw, long long ldc,
                                       long long ldr, float alpha, int act, void* stream) {
  return kfamd_gemm_nt_skinny_w8_tiles(0, 0, A, codes, wscale, C, bias, R, M, N, K, lda, ldw, ldc, ldr, alpha, act,
                                       stream);
}

// ---- gated (SwiGLU) entry points: codes [N = 2F][K] interleaved (row 2j gate, 2j + 1 up), C [M][F] ------------
extern "C" int kfamd_gemm_nt_skinny_w8_glu_tiles(int path, int tiles, const void* A, const void* codes,
                                                 const float* wscale, void* C, const void* bias, int M, int N, int K,
                                                 long long lda, long long ldw, long long ldc, float alpha,
                                                 void* stream) {
  return w8_launch<true>(path, tiles, A, codes, wscale, C, bias, nullptr, M, N, K, lda, ldw, ldc, 0, alpha,
                         KFAMD_ACT_NONE, stream);
}

extern "C" int kfamd_gemm_nt_skinny_w8_glu_path(int path, const void* A, const void* codes, const float* wscale,
                                                void* C, const void* bias, int M, int N, int K, long long lda,
                                                long long ldw, long long ldc, float alpha, void* stream) {
  return kfamd_gemm_nt_skinny_w8_glu_tiles(path, 0, A, codes, wscale, C, bias, M, N, K, lda, ldw, ldc, alpha, stream);
}

extern "C" int kfamd_gemm_nt_skinny_w8_glu(const void* A, const void* codes, const float* wscale, void* C,
                                           const void* bias, int M, int N, int K, long long lda, long long ldw,
                                           long long ldc, float alpha, void* stream) {
  return kfamd_gemm_nt_skinny_w8_glu_tiles(0, 0, A, codes, wscale, C, bias, M, N, K, lda, ldw, ldc, alpha, stream);
}
