// gemm_fp8.hip — dense W8A8 FP8 NT GEMM for prefill and chunk steps, and the activation quantiser that feeds it.
//   C[m][n] = act(alpha * sa[m] * sw[n] * sum_k ca[m][k] * cw[n][k] + bias[n]) + R[m][n]
// (the rule: ops/gemm.py's docstring). ca [M][K] and cw [N][K] are OCP e4m3fn codes, K contiguous, with one fp32
// scale per row (ops.QuantizedWeight, the format of ops.decode.quantize_rows); bias, R and C are bf16; the sum is
// fp32 on v_mfma_f32_32x32x64_f8f6f4 and the result is rounded once, RNE, to bf16.
//
// One template, gemm_fp8_nt<WT>, over the 32x32 MFMA tiles a wave owns in each direction: WT = 4 is the large plan
// (256 x 256 output tile per workgroup, 128 x 128 per wave), WT = 2 the small one (128 x 128, 64 x 64 per wave).
//   Work split: a workgroup of 4 waves, 2 x 2 over its output tile. The WEIGHTS are the MFMA's A operand (the
//     32-"row" side) and the activations its B operand: in the 32x32 result layout a lane then holds, for ONE
//     activation row m = lane & 31, the weight rows 8 g + 4 (lane >> 5) + 0..3 (g = 0..3): four consecutive n of one
//     output row, stored as one 8-byte piece where the pointers allow (C, bias, R 8-B aligned, ldc % 4 == ldr % 4
//     == 0, sw 16-B aligned; bias, R and sw are then read as one piece too), else element by element.
//     Accumulators: WT^2 x 16 fp32 per lane (256 at WT = 4, 64 at WT = 2).
//   Operands: an f8f6f4 MFMA takes 64 k per instruction; lane l supplies 32 contiguous K bytes (k-half l >> 5) of
//     operand row l & 31: two 16-byte LDS reads, no transposing read. Both operands use the same mapping, so the dot
//     product does not depend on how the instruction orders the 64 k internally.
//   K step: 128 bytes (two MFMA k-steps). Per step a wave reads 2 WT fragments per k-half step and issues WT^2 MFMAs
//     on them (4 x 4 x 2 = 32 MFMAs against 32 ds_read_b128 at WT = 4).
//   Data movement: global -> registers -> LDS, a ring of 2 stages. Thread t loads the 16-byte chunk t & 7 of rows
//     t / 8 + 32 j (j < 2 WT) of each operand image with range-checked raw buffer loads (8 lanes cover one 128-byte
//     line of a row). The loads of K step kt + 1 are issued BEFORE the MFMAs of step kt and written to the other
//     stage after them; one barrier per K step (a stage is overwritten only after the barrier that follows its last
//     read).
//   LDS image: rows of 128 bytes, no padding; the 16-byte chunk c of row r sits at chunk position c ^ ((r >> 1) & 7).
//     The LDS has 64 banks of 4 bytes (256 bytes per pass), and a ds_read_b128 / ds_write_b128 is served 16 lanes at
//     a time. A fragment read: 16 consecutive lanes are 16 consecutive rows r at the same chunk c; rows 2 i and 2 i + 1
//     share the XOR term and lie in the two 128-byte halves of one 256-byte span, and the 8 row pairs get 8 distinct
//     positions: 16 distinct 16-byte slots of the 256, conflict-free. A write: 16 lanes are two consecutive rows x 8
//     chunks, again the two halves x a permutation of the 8 positions: conflict-free.
//   LDS budget: 2 stages x 2 operands x (64 WT rows x 128 B) = 128 KB at WT = 4 (one workgroup, 4 waves, per CU of
//     160 KB) and 64 KB at WT = 2 (two workgroups per CU).
//   Edges, in the kernel: any M, N >= 1 and K % 16 == 0. A chunk whose row is at or past M / N, or whose bytes are at
//     or past K, gets a buffer offset beyond num_records and reads as zero (FP8 code 0 is +0): it is never read as
//     data, whatever lies there (the host keeps (rows - 1) * ld + K below 2^31). Stores are masked by m < M, n < N. No
//     pad or transpose copies.
//   Epilogue: fp32, in the rule's order: x (alpha * sa[m]) x sw[n], + bias, activation, + residual, one rounding.
//     No atomics, no split-K: a captured launch replays its bits.
//   Plan (kfamd_gemm_nt_fp8, plan = 0): the small tile, always. The first rule (large from 128 workgroups, half of
//     the 256 CUs) lost to the forced small tile at every measured shape where it chose the large one
//     (profiles/w8a8/README.md), so the large tile is kept for plan = 1 only until it wins somewhere; plan = 1 / 2
//     force large / small.
//
// quantize_rows_bf16: bf16 rows [M][K] (any row stride) -> e4m3fn codes [M][K] + fp32 scale [M], bit for bit
//   ops.decode.quantize_rows: scale = amax / 448 (1 for a zero row), code = RNE_e4m3(clamp(x / scale, -448, 448)),
//   IEEE divisions as kv_append_fp8 (attn_kv.hip). One wave per row, two passes over it (the second hits L2): amax
//   by kfw::wave_max, then 8 elements per lane and step, one 8-byte code store each.
//
// Registers (gfx950, -Rpass-analysis=kernel-resource-usage; the build refuses scratch in this file): see
// profiles/w8a8/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBK = 128;                 // K bytes per step
constexpr unsigned kOOB = 0x80000000u;   // buffer offset of a chunk that reads as zero
constexpr float kFp8Max = 448.f;

// 0.5 v (1 + tanh(u)) == v * sigmoid(2 u): one v_exp_f32 per value and no branch per activation code, so that the
// epilogue unrolls over the accumulators (a libm tanhf there kept it a loop, with the accumulators in scratch)
__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == KFAMD_ACT_NONE) return v;
  if (act == KFAMD_ACT_RELU) return v > 0.f ? v : 0.f;
  const float u = act == KFAMD_ACT_GELU_TANH ? 1.5957691216057308f * (v + 0.044715f * v * v * v) : v;
  return v / (1.f + __expf(-u));
}

struct Fp8Args {
  const uint8_t* A;   // activation codes [M][lda]
  const uint8_t* W;   // weight codes [N][ldw]
  const float* sa;    // [M]
  const float* sw;    // [N]
  __bf16* C;
  const __bf16* bias;
  const __bf16* R;
  int M, N, K;
  long long lda, ldw, ldc, ldr;
  float alpha;
  int act;
  int vec;  // at columns that are multiples of 4: C, bias and R rows take 8-byte accesses, sw 16-byte loads
};

// byte offset of 16-byte chunk c of row r in a [rows][128 B] LDS image (header: the swizzle)
__device__ __forceinline__ int img_off(int r, int c) { return r * kBK + ((c ^ ((r >> 1) & 7)) << 4); }

template <int WT>  // 2 or 4
__global__ __launch_bounds__(256) void gemm_fp8_nt(Fp8Args a) {
  constexpr int BT = 64 * WT;        // tile rows, along m and along n
  constexpr int PIECES = BT / 32;    // 16-byte chunks per thread, operand image and K step
  constexpr int IMG = BT * kBK;      // bytes of one operand image
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * IMG];  // [stage][W image | A image]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_n = (a.N + BT - 1) / BT;
  const int n_tile = (blockIdx.x % tiles_n) * BT, m_tile = (blockIdx.x / tiles_n) * BT;

  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.W), (short)0, (int)((a.N - 1) * a.ldw + a.K), 0x00020000);
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.A), (short)0, (int)((a.M - 1) * a.lda + a.K), 0x00020000);

  // the chunks this thread moves: chunk lc of rows lr + 32 j
  const int lr = tid >> 3, lc = tid & 7;
  unsigned woff[PIECES], aoff[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int n = n_tile + lr + 32 * j, m = m_tile + lr + 32 * j;
    woff[j] = n < a.N ? (unsigned)(n * a.ldw) + lc * 16 : kOOB;
    aoff[j] = m < a.M ? (unsigned)(m * a.lda) + lc * 16 : kOOB;
  }

  u32x4 gw[PIECES], ga[PIECES];
  auto load_global = [&](int kt) __attribute__((always_inline)) {
    const int k0 = kt * kBK;
    const bool kin = k0 + lc * 16 < a.K;  // K % 16 == 0: a chunk lies wholly inside or outside K
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      gw[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            rw, (int)(kin && woff[j] != kOOB ? woff[j] + k0 : kOOB), 0, 0));
      ga[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            ra, (int)(kin && aoff[j] != kOOB ? aoff[j] + k0 : kOOB), 0, 0));
    }
  };
  auto store_lds = [&](int stage) __attribute__((always_inline)) {
    char* base = smem + stage * 2 * IMG;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int off = img_off(lr + 32 * j, lc);
      *reinterpret_cast<u32x4*>(base + off) = gw[j];
      *reinterpret_cast<u32x4*>(base + IMG + off) = ga[j];
    }
  };

  f32x16 acc[WT][WT];  // [mi][ni]
#pragma unroll
  for (int mi = 0; mi < WT; ++mi)
#pragma unroll
    for (int ni = 0; ni < WT; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int wm = (wave >> 1) * (32 * WT), wn = (wave & 1) * (32 * WT);  // the wave's corner inside the tile
  const int fr = lane & 31, fh = lane >> 5;                             // fragment row, k-half

  auto frag = [&](const char* img, int row, int ks) __attribute__((always_inline)) {
    const int c = ks * 4 + fh * 2;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(img + img_off(row, c));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(img + img_off(row, c + 1));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };

  const int nk = (a.K + kBK - 1) / kBK;
  load_global(0);
  store_lds(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;  // workgroup-uniform
    if (more) load_global(kt + 1);
    const char* wimg = smem + (kt & 1) * 2 * IMG;
    const char* aimg = wimg + IMG;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      i32x8 fw[WT], fa[WT];
#pragma unroll
      for (int i = 0; i < WT; ++i) {
        fw[i] = frag(wimg, wn + 32 * i + fr, ks);
        fa[i] = frag(aimg, wm + 32 * i + fr, ks);
      }
#pragma unroll
      for (int mi = 0; mi < WT; ++mi)
#pragma unroll
        for (int ni = 0; ni < WT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[ni], fa[mi], acc[mi][ni], 0, 0, 0, 0, 0, 0);
    }
    if (more) store_lds((kt + 1) & 1);
    __syncthreads();
  }

  // epilogue. acc[mi][ni][4 g + i]: activation row m_tile + wm + 32 mi + fr, weight row n_tile + wn + 32 ni + 8 g +
  // 4 fh + i
  // (one call per mi, its index a constant: as ONE unrolled loop nest the epilogue passes the compiler's size limit
  // for unrolling, stays a loop and indexes the accumulators through scratch)
  auto epilogue = [&](auto mi_c) __attribute__((always_inline)) {
    constexpr int mi = decltype(mi_c)::value;
    const int m = m_tile + wm + 32 * mi + fr;
    if (m >= a.M) return;
    const float am = a.alpha * a.sa[m];
#pragma unroll
    for (int ni = 0; ni < WT; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int nb = n_tile + wn + 32 * ni + 8 * g + 4 * fh;
        if (nb < a.N) {
          float v[4];
          __bf16* c = a.C + m * a.ldc + nb;
          if (a.vec && nb + 3 < a.N) {  // the four n of a piece in one load each: sw 16 bytes, bias / R / C 8 bytes
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(a.sw + nb);
            bf16x4 b4 = {}, r4 = {};
            if (a.bias) b4 = *reinterpret_cast<const bf16x4*>(a.bias + nb);
            if (a.R) r4 = *reinterpret_cast<const bf16x4*>(a.R + m * a.ldr + nb);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              v[i] = acc[mi][ni][4 * g + i] * am * s4[i];
              if (a.bias) v[i] += (float)b4[i];
              v[i] = apply_act(v[i], a.act);
              if (a.R) v[i] += (float)r4[i];
            }
            *reinterpret_cast<bf16x4*>(c) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int n = min(nb + i, a.N - 1);
              v[i] = acc[mi][ni][4 * g + i] * am * a.sw[n];
              if (a.bias) v[i] += (float)a.bias[n];
              v[i] = apply_act(v[i], a.act);
              if (a.R) v[i] += (float)a.R[m * a.ldr + n];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (nb + i < a.N) c[i] = (__bf16)v[i];
          }
        }
      }
  };
  epilogue(std::integral_constant<int, 0>{});
  epilogue(std::integral_constant<int, 1>{});
  if constexpr (WT == 4) {
    epilogue(std::integral_constant<int, 2>{});
    epilogue(std::integral_constant<int, 3>{});
  }
}

// one wave per row, 4 rows per workgroup
__global__ __launch_bounds__(256) void quantize_rows_bf16(const __bf16* __restrict__ x, uint8_t* __restrict__ codes,
                                                          float* __restrict__ scale, int M, int K, long long ldx,
                                                          long long ldq) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  const __bf16* xr = x + row * ldx;
  float am = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const u32x4 p = *reinterpret_cast<const u32x4*>(xr + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      am = fmaxf(am, fabsf(__uint_as_float(p[i] << 16)));
      am = fmaxf(am, fabsf(__uint_as_float(p[i] & 0xffff0000u)));
    }
  }
  am = kfw::wave_max(am);
  const float s = am > 0.f ? am / kFp8Max : 1.f;  // IEEE division: the torch reference's scale
  if (lane == 0) scale[row] = s;
  uint8_t* qr = codes + row * ldq;
  for (int k = lane * 8; k < K; k += 512) {
    const u32x4 p = *reinterpret_cast<const u32x4*>(xr + k);
    float y[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[2 * i] = __uint_as_float(p[i] << 16);
      y[2 * i + 1] = __uint_as_float(p[i] & 0xffff0000u);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(y[i] / s, -kFp8Max), kFp8Max);
    u32x2 w;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int q = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i], y[4 * i + 1], 0, false);
      q = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i + 2], y[4 * i + 3], q, true);
      w[i] = (unsigned)q;
    }
    *reinterpret_cast<u32x2*>(qr + k) = w;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int kfamd_gemm_nt_fp8_plan(int M, int N) {
  if (M < 1 || N < 1) return KFAMD_EINVAL;
  return 2;  // measured (profiles/w8a8): the 128 x 128 tile equals or beats the 256 x 256 one at every shape
}

extern "C" int kfamd_gemm_nt_fp8(int plan, const void* a_codes, const float* a_scale, const void* w_codes,
                                 const float* w_scale, void* C, const void* bias, const void* R, int M, int N, int K,
                                 long long lda, long long ldw, long long ldc, long long ldr, float alpha, int act,
                                 void* stream) {
  if (!a_codes || !a_scale || !w_codes || !w_scale || !C) return KFAMD_EINVAL;
  if (M < 1 || N < 1 || K < 16 || K % 16 || plan < 0 || plan > 2) return KFAMD_EINVAL;
  if (act < KFAMD_ACT_NONE || act > KFAMD_ACT_SILU) return KFAMD_EINVAL;
  if (lda < K || ldw < K || ldc < N || (R && ldr < N)) return KFAMD_EINVAL;
  // 32-bit buffer offsets, and the zero-fill offset must lie beyond every record
  if ((M - 1) * lda + K > 0x7fffffffLL || (N - 1) * ldw + K > 0x7fffffffLL) return KFAMD_EINVAL;
  if (!al16(a_codes) || !al16(w_codes) || (lda & 15) || (ldw & 15)) return KFAMD_EALIGN;
  Fp8Args a;
  a.A = static_cast<const uint8_t*>(a_codes);
  a.W = static_cast<const uint8_t*>(w_codes);
  a.sa = a_scale, a.sw = w_scale;
  a.C = static_cast<__bf16*>(C);
  a.bias = static_cast<const __bf16*>(bias);
  a.R = static_cast<const __bf16*>(R);
  a.M = M, a.N = N, a.K = K;
  a.lda = lda, a.ldw = ldw, a.ldc = ldc, a.ldr = ldr;
  a.alpha = alpha;
  a.act = act;
  const auto al = [](const void* p, int b) { return (reinterpret_cast<uintptr_t>(p) & (b - 1)) == 0; };
  a.vec = al(C, 8) && (ldc & 3) == 0 && al(w_scale, 16) && al(bias, 8) && al(R, 8) && (!R || (ldr & 3) == 0);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int p = plan ? plan : kfamd_gemm_nt_fp8_plan(M, N);
  const int bt = p == 1 ? 256 : 128;
  const long long tiles = (long long)((M + bt - 1) / bt) * ((N + bt - 1) / bt);
  if (tiles > 0x7fffffffLL) return KFAMD_EINVAL;
  if (p == 1) hipLaunchKernelGGL((gemm_fp8_nt<4>), dim3((unsigned)tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_fp8_nt<2>), dim3((unsigned)tiles), dim3(256), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

extern "C" int kfamd_quantize_rows_bf16(const void* x, void* codes, float* scale, int M, int K, long long ldx,
                                        long long ldq, void* stream) {
  if (!x || !codes || !scale || M < 1 || K < 8 || K % 8 || ldx < K || ldq < K) return KFAMD_EINVAL;
  if (!al16(x) || (ldx & 7) || (reinterpret_cast<uintptr_t>(codes) & 7) || (ldq & 7)) return KFAMD_EALIGN;
  hipLaunchKernelGGL(quantize_rows_bf16, dim3((unsigned)((M + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), static_cast<const __bf16*>(x),
                     static_cast<uint8_t*>(codes), scale, M, K, ldx, ldq);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}
