// gemm_skinny_mx4.hip — weight-streaming NT GEMM on OCP MXFP4 weights (4.25 bits per weight) for decode:
//   C[M][N] = act(alpha * (A[M][K] . W[N][K]^T) + bias[n]) (+ R[M][N]),  1 <= M <= 16,  K % 32 == 0.
// A, bias, R, C are bf16, accumulation fp32. W is the dequantised weight of ops.MXFP4Weight (kubeflow_rm_amd/ops/
// gemm.py states the format once; this file follows it): codes [N][K / 2] bytes, row stride ldw BYTES, element 2i in
// the low nibble of byte i and 2i + 1 in the high one, e2m1; scales [N][K / 32] bytes, row stride lds, e8m0, one per
// group of 32 elements, byte e in [1, 254] meaning 2^(e - 127). Every e2m1 value times a power of two is a bf16
// value, so the widened operand IS the dequantised weight: the products are exact as in gemm_skinny_bf16.hip, there
// is no per-group fix-up of partial sums and no row scale in the epilogue. Scale bytes 0 and 255 and magnitudes
// below 2^-126 are out of contract.
//
// The design is the skeleton gemm_skinny_bf16.hip and gemm_skinny_w8.hip share: the codes are read exactly once from
// HBM in 16-B loads straight to VGPRs, no LDS staging of weights, the loads of several K chunks issued before the
// first is consumed, a fixed summation order and no atomics (deterministic, capturable). Nothing dequantised is
// written to memory. What the format changes: a 16-B piece is one whole MX group, 32 k-elements and one scale.
//   Widening: v_cvt_scalef32_pk_bf16_fp4 (the builtin, four byte selects per dword: 4 converts per 8 codes, no
//     v_perm) turns one byte and the fp32 scale (e << 23) into a bf16 pair, low nibble first: the format's order, so
//     dword j of a piece becomes the bf16x8 fragment of elements 8j .. 8j + 7 as it stands. The VALU form uses
//     v_cvt_scalef32_pk_f32_fp4 the same way.
//   MFMA (skinny_mx4_mfma<TILES>): a 256-thread workgroup owns TILES x 8 weight rows and splits K over its 4 waves
//     in 256-element chunks. Per chunk a wave loads 8 rows x 128 B (full lines: lane l = row l & 7, piece l >> 3) and
//     widens each piece into four bf16x8 fragments f0 .. f3. As the 16-row operand of v_mfma_f32_16x16x32_bf16
//     (operand row r = lane & 15, k-slot q = lane >> 4), fragment fj of operand row r holds weight row r & 7 at
//     k = 64q + 32 (r >> 3) + 8j of the chunk. So the eight 8-element activation pieces a lane needs are the 64
//     contiguous elements 64q .. 64q + 63 of its activation row (b0 .. b7, 128 B), and a tile and chunk cost eight
//     MFMAs: fj x bj into acc_e (operand rows 0-7 valid) and fj x b(4 + j) into acc_o (rows 8-15 valid), j = 0 .. 3.
//     Half-valid accumulators are accepted: the kernel is a byte stream. Reduction over the waves through LDS and
//     epilogue as in the W8 kernel.
//   Scales, MFMA form: a chunk needs 8 contiguous scale bytes per row. The 8 lanes that share a weight row issue one
//     8-byte load of the same address (one request per row, issued with the chunk's code loads so that both share
//     the latency) and each picks byte lane >> 3. The scale rows are K / 32 bytes apart, so the address has no
//     alignment (an unaligned global_load_dwordx2). In the tail chunk the window is moved back to the row's last 8
//     bytes and the byte index shifted, so no load leaves the row; a row of fewer than 8 scale bytes (K < 256, one
//     chunk in all) is read by one byte load per lane.
//   VALU (skinny_mx4_valu<MR, ROWS>): a wave owns ROWS weight rows over the whole K; lane l takes the 16-B pieces
//     l, l + 64, ... of every row, their scale bytes (lane l byte l: one coalesced 64-byte request per row) and the
//     matching 64 B of the MR activation rows; codes -> fp32, 32 * MR FMAs per piece, the ROWS * MR sums meet in
//     wave_sum.
//   K tail: K % 32 == 0, so a piece lies wholly inside or wholly outside K. Outside pieces are zero in both operands
//     with the address clamped and the scale forced to 1.
//
// Cut-over (kfamd_gemm_nt_skinny_mx4, path 0): the VALU form at M <= 2 (kValuMaxM) below N = kValuMaxN, the MFMA form
// everywhere else. Measured on the gpt-1b shapes with both forms and every tile / row count forced at M = 1, 2, 4, 8,
// 16 (tools/decode_bench.py --steps mx4, profiles/mx4/README.md; medians of 7 interleaved blocks, us per call from
// Python, so 10 - 11 us is the launch floor and every N x 2048 shape below the LM head sits on it in both forms). What
// separates, VALU (2 / 4 rows per wave) / MFMA (best TILES):
//   2048x8192: M = 1 11.5 / 11.2 against 11.4, M = 2 11.2 / 11.3 against 11.1 (level), M = 4 15.1 / 14.2 against
//     11.0, M = 8 23.4 / 23.4 against 11.6;
//   8192x2048 and 6144x2048: level to M = 4; M = 8 17.1 / 17.1 against 11.0 and 14.5 / 14.4 against 11.1;
//   32000x2048: M = 1 16.4 / 14.9 against 14.0, M = 2 26.3 / 24.9 against 14.2, M = 8 59.0 against 14.7.
// Per call the two forms are level at M <= 2 below the LM head, because both sit on the launch floor; a captured
// graph has no such floor, and there the VALU form is the faster one: the graphed gpt-1b decode step at B = 1 takes
// 1.14 ms/token with the VALU form at M <= 2 and 1.31 with the MFMA form at every M (FP8 weights: 1.22). So M <= 2
// takes the VALU form below N = 16384, M = 4 does not (it loses at 2048x8192), and the LM head stays on the MFMA form
// at every M, as in the W8 kernel. The VALU instantiations for 4 and 8 activation rows are reached through
// kfamd_gemm_nt_skinny_mx4_path / _tiles only: kept so that this can be measured again. Tile counts by N, forced
// (us at TILES 1 / 2 / 4): 32000x2048 M = 1 20.8 / 17.6 / 14.0, M = 16 47.1 / 31.1 / 20.7; 8192x2048 M = 16 15.2 /
// 11.4 / 11.1, level at M <= 8; 6144x2048 and 2048x2048 level; 2048x8192 M = 1 11.4 / 15.3 / 24.7 (too few
// workgroups). Hence the W8 kernel's thresholds hold: TILES = 1 below N = 4096, 2 below 16384, 4 from there. Gated
// form (N = 2F, K = 2048; TILES 1 / 2 / 4): N = 16384 M = 8 15.5 / 13.8 / 12.9, M = 16 25.6 / 18.3 / 13.1; N = 11008
// M = 16 19.6 / 13.2 (13.2 - 13.5) / 12.7 (12.4 - 14.9), level below: the W8 kernel's rule (TILES = 4 from N = 8192
// above 8 activation rows) is kept. VALU weight rows per wave: 2 below N = 8192, 4 from there (level at M <= 2).
//
// Gated form (GLU template parameter, kfamd_gemm_nt_skinny_mx4_glu*): the same kernels with the SwiGLU epilogue over
// interleaved (gate, up) rows (ops/swiglu.py's layout rule), see glu_store.
//
// Registers (gfx950 compile, -Rpass-analysis=kernel-resource-usage; 0 scratch bytes in every instantiation, which
// the build checks; VGPRs / AGPRs, the gated instantiations within 3 of these): skinny_mx4_mfma<1> 110 / 8,
// <2> 119 / 16, <4> 96 / 32 (U = 1); skinny_mx4_valu<MR, ROWS>: <1,2> 120 / 0, <2,2> 134 / 0, <4,2> 77 / 0 (U = 1),
// <8,2> 121 / 0 (U = 1), <1,4> 165 / 0, <2,4> 187 / 0, <4,4> 126 / 0 (U = 1).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the cut-overs (header comment)
constexpr int kValuMaxM = 2;
constexpr int kGluValuMaxM = 2;
constexpr int kGluWideN = 8192;  // from here more than 8 activation rows take TILES = 4 (ungated: from N = 16384)
constexpr int kValuMaxN = 16384;

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

// an e8m0 scale byte (1 .. 254) as the converts' fp32 operand
__device__ __forceinline__ float e8m0(unsigned e) { return __uint_as_float(e << 23); }

// 8 e2m1 codes (one dword, memory order: low nibble of byte 0 first) times the group scale -> fp32
__device__ __forceinline__ void codes8(unsigned w, float s, float* f) {
  const f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 0);
  const f32x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 1);
  const f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 2);
  const f32x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 3);
  f[0] = p0[0], f[1] = p0[1], f[2] = p1[0], f[3] = p1[1], f[4] = p2[0], f[5] = p2[1], f[6] = p3[0], f[7] = p3[1];
}

// the same -> 8 bf16, exact
__device__ __forceinline__ bf16x8 codes8_bf16(unsigned w, float s) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

struct Mx4Args {
  const __bf16* A;
  const uint8_t* W;  // e2m1 codes [N][ldw bytes], two per byte
  const uint8_t* S;  // e8m0 scales [N][lds], one per 32 elements
  __bf16* C;
  const __bf16* bias;
  const __bf16* R;
  int M, N, K;
  long long lda, ldw, lds, ldc, ldr;
  float alpha;
  int act;
};

__device__ __forceinline__ void epilogue_store(const Mx4Args& a, int m, int n, float acc) {
  float v = acc * a.alpha;
  if (a.bias) v += (float)a.bias[n];
  v = apply_act(v, a.act);
  if (a.R) v += (float)a.R[m * a.ldr + n];
  a.C[m * a.ldc + n] = (__bf16)v;
}

// GLU (the gated form, kfamd_gemm_nt_skinny_mx4_glu*): as in gemm_skinny_bf16.hip, weight rows n (even) and n + 1
// are gate and up of output column n / 2
__device__ __forceinline__ void glu_store(const Mx4Args& a, int m, int n, float accg, float accu) {
  float g = accg * a.alpha, u = accu * a.alpha;
  if (a.bias) {
    g += (float)a.bias[n];
    u += (float)a.bias[n + 1];
  }
  a.C[m * a.ldc + (n >> 1)] = (__bf16)(g / (1.f + __expf(-g)) * u);
}

// ---- VALU form -------------------------------------------------------------------------------
template <int MR, int ROWS, bool GLU = false>
__global__ __launch_bounds__(256) void skinny_mx4_valu(Mx4Args a) {
  constexpr int U = MR >= 4 ? 1 : 2;  // 16-B pieces per row in flight per lane (64 * MR activation bytes each)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= a.N) return;  // wave-uniform; no barrier in this kernel
  const int pieces = a.K / 32;
  float acc[ROWS][MR];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;
  const uint8_t *wrow[ROWS], *srow[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const long long row = min(n0 + r, a.N - 1);
    wrow[r] = a.W + row * a.ldw;
    srow[r] = a.S + row * a.lds;
  }
  const __bf16* arow[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) arow[m] = a.A + (long long)min(m, a.M - 1) * a.lda;

  for (int p0 = 0; p0 < pieces; p0 += 64 * U) {
    u32x4 w[U][ROWS], x[U][MR][4];
    unsigned e[U][ROWS];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * 64 + lane;
      ok[u] = p < pieces;
      const int pc = ok[u] ? p : 0;  // a clamped (valid) address; its products are not accumulated
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        w[u][r] = *reinterpret_cast<const u32x4*>(wrow[r] + pc * 16);
        e[u][r] = srow[r][pc];
      }
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int h = 0; h < 4; ++h) x[u][m][h] = *reinterpret_cast<const u32x4*>(arow[m] + pc * 32 + h * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int h = 0; h < 4; ++h) {  // the piece's codes 8h .. 8h + 7
        float xf[MR][8];
#pragma unroll
        for (int m = 0; m < MR; ++m) unpack8(x[u][m][h], xf[m]);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float wf[8];
          codes8(w[u][r][h], e8m0(e[u][r]), wf);
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
__global__ __launch_bounds__(256) void skinny_mx4_mfma(Mx4Args a) {
  constexpr int U = TILES >= 4 ? 1 : 2;  // K chunks (256 elements) in flight per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * (8 * TILES);
  const int pieces = a.K / 32;  // 16-B code pieces = scale bytes per row
  const int nchunks = (pieces + 7) / 8;
  // W fragment: row lane & 7 of each tile, 16-B piece (32 codes, one scale) lane >> 3 of the chunk
  const int wpiece = lane >> 3;
  const uint8_t *wrow[TILES], *srow[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const long long row = min(n0 + t * 8 + (lane & 7), a.N - 1);
    wrow[t] = a.W + row * a.ldw;
    srow[t] = a.S + row * a.lds;
  }
  // activation fragments: row lane & 15 (clamped), elements 64q .. 64q + 63 of the chunk (128 contiguous bytes)
  const int q = lane >> 4;
  const __bf16* arow = a.A + (long long)min(lane & 15, a.M - 1) * a.lda;

  f32x4 acc_e[TILES], acc_o[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc_e[t] = acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};

  for (int c0 = wave; c0 < nchunks; c0 += 4 * U) {
    u32x4 w[U][TILES], x[U][8];
    float sc[U][TILES];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u * 4;
      const bool live = c < nchunks;  // wave-uniform
      // K % 32 == 0: a 32-code piece and each 8-element activation piece lie wholly inside or wholly outside K;
      // outside pieces are zero in BOTH operands (the address is clamped to the row's start, the scale is 1)
      const int p = c * 8 + wpiece;
      const bool wok = live && p < pieces;
      // the chunk's 8 scale bytes: a window of the row that never leaves it (moved back in the tail chunk)
      const int sbase = max(min(c * 8, pieces - 8), 0);
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(wrow[t] + (wok ? (long long)p * 16 : 0));
        w[u][t] = wok ? v : zero;
        unsigned e;
        if (pieces >= 8) {  // kernel-uniform
          unsigned long long s8;
          __builtin_memcpy(&s8, srow[t] + sbase, 8);
          e = (unsigned)(s8 >> (8 * ((p - sbase) & 7))) & 0xffu;
        } else {
          e = srow[t][wok ? p : 0];
        }
        sc[u][t] = wok ? e8m0(e) : 1.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int kx = c * 256 + q * 64 + i * 8;
        const bool xok = live && kx < a.K;
        const u32x4 v = *reinterpret_cast<const u32x4*>(arow + (xok ? kx : 0));
        x[u][i] = xok ? v : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bf16x8 b[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) b[i] = __builtin_bit_cast(bf16x8, x[u][i]);
#pragma unroll
      for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 f = codes8_bf16(w[u][t][j], sc[u][t]);
          acc_e[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, b[j], acc_e[t], 0, 0, 0);
          acc_o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, b[4 + j], acc_o[t], 0, 0, 0);
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
void launch_valu(const Mx4Args& a, int mr, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 4 * ROWS - 1) / (4 * ROWS))), block(256);
  switch (mr) {
    case 1: hipLaunchKernelGGL((skinny_mx4_valu<1, ROWS, GLU>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((skinny_mx4_valu<2, ROWS, GLU>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((skinny_mx4_valu<4, ROWS, GLU>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((skinny_mx4_valu<8, 2, GLU>), dim3((unsigned)((a.N + 7) / 8)), block, 0, s, a); break;
  }
}

template <int TILES, bool GLU>
void launch_mfma(const Mx4Args& a, hipStream_t s) {
  hipLaunchKernelGGL((skinny_mx4_mfma<TILES, GLU>), dim3((unsigned)((a.N + 8 * TILES - 1) / (8 * TILES))), dim3(256),
                     0, s, a);
}

template <bool GLU>
int mx4_launch(int path, int tiles, const void* A, const void* codes, const void* scales, void* C, const void* bias,
               const void* R, int M, int N, int K, long long lda, long long ldw, long long lds, long long ldc,
               long long ldr, float alpha, int act, void* stream) {
  if (!A || !codes || !scales || !C || M < 1 || M > 16 || N < 1 || K < 32 || K % 32) return KFAMD_EINVAL;
  if (GLU) {
    if ((N & 1) || ldc < N / 2) return KFAMD_EINVAL;
  } else {
    if (act < KFAMD_ACT_NONE || act > KFAMD_ACT_SILU || (R && act != KFAMD_ACT_NONE)) return KFAMD_EINVAL;
    if (ldc < N || (R && ldr < N)) return KFAMD_EINVAL;
  }
  if (lda < K || ldw < K / 2 || lds < K / 32) return KFAMD_EINVAL;
  if (path < 0 || path > 2 || (path == 1 && M > 8)) return KFAMD_EINVAL;
  const bool valu = path == 1 || (path == 0 && M <= (GLU ? kGluValuMaxM : kValuMaxM) && N < kValuMaxN);
  if (tiles != 0 && (valu ? (tiles != 2 && tiles != 4) : (tiles != 1 && tiles != 2 && tiles != 4))) return KFAMD_EINVAL;
  if (!al16(A) || !al16(codes) || (lda & 7) || (ldw & 15)) return KFAMD_EALIGN;
  Mx4Args a;
  a.A = static_cast<const __bf16*>(A);
  a.W = static_cast<const uint8_t*>(codes);
  a.S = static_cast<const uint8_t*>(scales);
  a.C = static_cast<__bf16*>(C);
  a.bias = static_cast<const __bf16*>(bias);
  a.R = static_cast<const __bf16*>(R);
  a.M = M, a.N = N, a.K = K;
  a.lda = lda, a.ldw = ldw, a.lds = lds, a.ldc = ldc, a.ldr = ldr;
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
extern "C" int kfamd_gemm_nt_skinny_mx4_tiles(int path, int tiles, const void* A, const void* codes,
                                              const void* scales, void* C, const void* bias, const void* R, int M,
                                              int N, int K, long long lda, long long ldw_bytes, long long lds,
                                              long long ldc, long long ldr, float alpha, int act, void* stream) {
  return mx4_launch<false>(path, tiles, A, codes, scales, C, bias, R, M, N, K, lda, ldw_bytes, lds, ldc, ldr, alpha,
                           act, stream);
}

extern "C" int kfamd_gemm_nt_skinny_mx4_path(int path, const void* A, const void* codes, const void* scales, void* C,
                                             const void* bias, const void* R, int M, int N, int K, long long lda,
                                             long long ldw_bytes, long long lds, long long ldc, long long ldr,
                                             float alpha, int act, void* stream) {
  return kfamd_gemm_nt_skinny_mx4_tiles(path, 0, A, codes, scales, C, bias, R, M, N, K, lda, ldw_bytes, lds, ldc, ldr,
                                        alpha, act, stream);
}

extern "C" int kfamd_gemm_nt_skinny_mx4(const void* A, const void* codes, const void* scales, void* C,
                                        const void* bias, const void* R, int M, int N, int K, long long lda,
                                        long long ldw_bytes, long long lds, long long ldc, long long ldr, float alpha,
                                        int act, void* stream) {
  return kfamd_gemm_nt_skinny_mx4_tiles(0, 0, A, codes, scales, C, bias, R, M, N, K, lda, ldw_bytes, lds, ldc, ldr,
                                        alpha, act, stream);
}

// ---- gated (SwiGLU) entry points: codes [N = 2F][K / 2] interleaved (row 2j gate, 2j + 1 up), C [M][F] ---------
extern "C" int kfamd_gemm_nt_skinny_mx4_glu_tiles(int path, int tiles, const void* A, const void* codes,
                                                  const void* scales, void* C, const void* bias, int M, int N, int K,
                                                  long long lda, long long ldw_bytes, long long lds, long long ldc,
                                                  float alpha, void* stream) {
  return mx4_launch<true>(path, tiles, A, codes, scales, C, bias, nullptr, M, N, K, lda, ldw_bytes, lds, ldc, 0, alpha,
                          KFAMD_ACT_NONE, stream);
}

extern "C" int kfamd_gemm_nt_skinny_mx4_glu_path(int path, const void* A, const void* codes, const void* scales,
                                                 void* C, const void* bias, int M, int N, int K, long long lda,
                                                 long long ldw_bytes, long long lds, long long ldc, float alpha,
                                                 void* stream) {
  return kfamd_gemm_nt_skinny_mx4_glu_tiles(path, 0, A, codes, scales, C, bias, M, N, K, lda, ldw_bytes, lds, ldc,
                                            alpha, stream);
}

extern "C" int kfamd_gemm_nt_skinny_mx4_glu(const void* A, const void* codes, const void* scales, void* C,
                                            const void* bias, int M, int N, int K, long long lda, long long ldw_bytes,
                                            long long lds, long long ldc, float alpha, void* stream) {
  return kfamd_gemm_nt_skinny_mx4_glu_tiles(0, 0, A, codes, scales, C, bias, M, N, K, lda, ldw_bytes, lds, ldc, alpha,
                                            stream);
}
