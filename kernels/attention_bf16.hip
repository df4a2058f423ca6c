// attention_bf16.hip — flash attention forward + backward for gfx950 (bf16 I/O, fp32 softmax).
//
// The in-notebook model's attention (models/gpt.py) without the N x N score matrix and without
// torch's aotriton (Triton-generated) kernels: every product runs on v_mfma_f32_32x32x16_bf16,
// the online softmax in fp32 registers, K/V tiles staged through a swizzled LDS image.
//
// Layout and lane maps (cdna_hip_programming.md §3, "An accumulator tile as the next MFMA's
// operand"): a 32x32 accumulator has its column on the lane (lane & 31) and its rows in the 16
// registers, row(reg, half) = (reg & 3) + 8 * (reg >> 2) + 4 * half. Every product is oriented
// so that the NEXT product sums over the accumulator's row index, which lets the accumulator
// (converted to bf16 pairwise) be that product's operand with no lane movement:
//
//   forward, per wave = 32 query rows, per 64-key tile:
//     S^T[key][q]  = K . Q^T          A = K rows (LDS, ds_read_b128), B = Q (registers)
//     O^T[d][q]   += V^T . P^T        A = V columns (LDS, ds_read_b64_tr_b16), B = P^T = the S^T
//                                     accumulator in bf16 (query on the lane: the online-softmax
//                                     max / sum / rescale of a row stay in its lane pair)
//   backward dK / dV (attn_bwd_dkdv8), per wave = 32 keys, per 32-query tile (keys on the lane):
//     S[q][key]   = Q . K^T - lse/scale    (the row constant preloaded into the accumulator)
//     dP[q][key]  = dO . V^T - delta       (delta = rowsum(dO * O), preloaded the same way)
//     dV^T[d][key] += dO^T . P             A = dO columns (tr reads), B = P accumulator
//     dK^T[d][key] += Q^T . dS             A = Q columns (tr reads),  B = dS accumulator
//   backward dQ (attn_bwd_dq_split, runs first), per wave = 32 query rows, per 64-key tile, as the
//   forward: S^T and dP^T recomputed with the query on the lane, dS^T the B operand of
//     dQ^T[d][q]  += K^T . dS^T            A = K columns (tr reads); written once as bf16, no atomics.
//   It also computes delta and writes both row constants for the dK / dV kernel.
//
// LDS images: one swizzle per head dim serves both the row reads (ds_read_b128 of a 16-B chunk
// by 32 different rows) and the transposed reads (ds_read_b64_tr_b16 of 4 consecutive rows by 32
// columns) without bank conflicts (T2 / T10): 16-B chunk ch of row r sits at chunk
//   D = 128 (256-B rows): ch ^ (((r & 3) << 2) | ((r >> 2) & 3))
//   D =  64 (128-B rows): ch ^ g((r >> 1) & 7),  g(x) = ((x & 1) << 2) | (x >> 1)
//
// Tensors are [B][H][T][D] views with element strides (b, h, t) and a contiguous head dim, so the
// fused QKV projection output [B][T][3][H][D] is read in place and the output / gradients are
// written straight into [B][T][H][D] / [B][T][3][H][D] (no transposes around the kernel).
// Causal masking is key <= query. The forward's workgroups run heaviest query block first; the
// backward's key blocks are heaviest first already (block 0 sees every query).
//
// Grouped-query attention (AttnShape::Hkv < H): K / V (and dK / dV) have Hkv heads and query head h
// reads head h / G, G = H / Hkv, in place. The forward and dQ kernels change only their K / V base
// offsets: grids, kernel choice, pairing and block_order stay in query heads, so a head computes
// what it computes on expanded K / V, bit for bit. block_order gives an XCD consecutive heads, so a
// group's K / V tiles meet in one L2 whenever G divides the heads per XCD (B H / 8). dK / dV sums a
// group in fp32 inside attn_bwd_dkdv8 (GRP), see there and gqa_group_split.
//
// Counterpart in the reference: none (its notebook images ship the framework's own attention);
// SURVEY §7.1C rules out Triton on the hot path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_tile.h"
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

using namespace kfa;  // the LDS tile image, its reads, mfma32, pack2, buffer loads: attn_tile.h

constexpr float kLog2e = 1.4426950408889634f;

struct AttnShape {
  int B, H, T;
  float scale;
  // grouped-query attention: Hkv K / V heads, G = H / Hkv query heads per K / V head (1: every head its own);
  // GS: the query heads of a group that one dK / dV workgroup sweeps (a divisor of G; attn_bwd_dkdv8 GRP)
  int Hkv, G, GS;
  // element strides (b, h, t) of q, k, v, o, do, dq, dk, dv
  long long s[8][3];
};

enum { TQ = 0, TK = 1, TV = 2, TO = 3, TDO = 4, TDQ = 5, TDK = 6, TDV = 7 };

__device__ __forceinline__ long long base_off(const AttnShape& a, int t, int b, int h) {
  return b * a.s[t][0] + h * a.s[t][1];
}

// bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"): the
// blocks dealt to one XCD (bid % 8 equal) get consecutive logical ids, so a head's blocks share L2
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Work order (profiles/r5zb_attn_lpt). A causal pass's blocks differ in work: query block i of the forward sees
// i + 1 key tiles, key block i of the backward sees the queries from i on. The hardware deals
// workgroups to the 8 XCDs round-robin (bid % 8) and each XCD starts its share in bid order, so a
// head-major order left the heaviest blocks of an XCD's last heads to start when the rest was done
// (makespan 1.5x the mean at 8 heads x 16 blocks on an XCD's 64 slots). Here XCD x owns heads
// [x BH/8, (x+1) BH/8) and walks them in groups of G heads, the fewest whose blocks fill its slots:
// the heaviest rank of every head of the group first (longest-processing-time order), the group's
// K / V shared in the XCD's L2. rank 0 = the heaviest block. Other head counts: the plain order.
struct BlockId {
  int bh, rank;
};
__device__ __forceinline__ BlockId block_order(int bid, int nblk, int BH, int slots) {
  if ((BH & 7) == 0) {
    const int hpx = BH >> 3, xcd = bid & 7, i = bid >> 3;
    int G = 1;
    while (G < hpx && (G * nblk < slots || hpx % G != 0)) ++G;
    const int gs = G * nblk, g = i / gs, j = i - g * gs;
    return {xcd * hpx + g * G + j % G, j / G};
  }
  const int nwg = nblk * BH;
  const int lid = (nwg & 7) == 0 ? xcd_remap(bid, nwg) : bid;
  return {lid / nblk, lid % nblk};
}

// Row-guarded loads are raw buffer operations over one (b, h) slice whose range ends at row T
// (slice_rsrc / bload16, slice_desc / dma16): a row past T reads as zero by the address unit, so the
// inner loops carry no per-row branches (a divergent `if (row < T)` around each load split
// the loops into ~30 basic blocks and cost the scheduler and the register allocator;
// profiles/r5o_attn_buf). The host requires every slice's extent below 2^31 bytes (32-bit buffer
// offsets): slice_ok.
//
// LDS-DMA as inline asm: the compiler, seeing a buffer_load ... lds builtin, waits
// vmcnt(0) before later LDS reads it cannot prove disjoint (it did, mid-tile, before the dV / dK tr
// reads: the next tile's DMA latency exposed). The kernel's own waits cover the pieces instead.
// The descriptor is an SGPR quad (base, base_hi | stride 0, records, gfx9 raw-buffer word 3); M0 holds
// the wave's 1 KiB LDS destination (lane L writes +16 L); s_nop 1 covers the M0 -> LDS-DMA hazard.
// (No compiler-generated code in this file uses M0: LDS instructions do not on gfx9+, and every
// LDS-DMA here is this asm, so M0 is not listed as clobbered — hipcc treats it as reserved.)
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 slice_desc(const void* base, long long bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  return i32x4{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffff)),
               (int)bytes, 0x00020000};
}
__device__ __forceinline__ unsigned lds_addr(const char* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
// voff: the lane's byte offset (VGPR); soff: a wave-uniform byte offset (SGPR: the tile's row offset,
// so the per-lane part is computed once outside the loop)
__device__ __forceinline__ void dma16(const i32x4& desc, unsigned lds, int voff, int soff = 0) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 1\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voff), "s"(desc),
                  "s"(__builtin_amdgcn_readfirstlane(soff)) : "memory");
}
__device__ __forceinline__ void dma4(const i32x4& desc, unsigned lds, int voff, int soff = 0) {  // lane L -> +4 L
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 1\n\tbuffer_load_dword %1, %2, %3 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voff), "s"(desc),
                  "s"(__builtin_amdgcn_readfirstlane(soff)) : "memory");
}

// Whole 16-B row stores of an accumulator in the O^T layout (cdna_hip_programming.md T21): lane
// (r, hh) holds row r's columns 32 n + 8 g + 4 hh .. +3 as acc[n][4 g .. 4 g + 3], g = 0..3. For each
// column-group pair (2k, 2k + 1) the lanes r and r + 32 trade halves with v_permlane32_swap, after
// which lane hh holds the 8 contiguous columns 8 (2k + hh) .. +7: 2 ND dwordx4 stores per lane
// instead of 4 ND dwordx2. Every lane must execute it (the swap needs EXEC full): `ok` guards only
// the stores (rows past T).
template <int ND>
__device__ __forceinline__ void store_rows16(__bf16* row, const f32x16 (&acc)[ND], float sc, bool ok, int hh) {
#pragma unroll
  for (int n = 0; n < ND; ++n)
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const int g0 = 2 * k2, g1 = g0 + 1;
      uint32_t p[2], q[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const auto sw = __builtin_amdgcn_permlane32_swap(pack2(acc[n][4 * g0 + 2 * x] * sc, acc[n][4 * g0 + 2 * x + 1] * sc),
                                                         pack2(acc[n][4 * g1 + 2 * x] * sc, acc[n][4 * g1 + 2 * x + 1] * sc),
                                                         false, false);
        p[x] = sw[0];
        q[x] = sw[1];
      }
      if (ok) *reinterpret_cast<u32x4*>(row + 32 * n + 8 * (g0 + hh)) = (u32x4){p[0], p[1], q[0], q[1]};
    }
}

// ------------------------------------------------------------------------------------------------
// forward: one workgroup = 4 waves = 128 query rows of one (b, h); 64-key K/V tiles through a
// double-buffered LDS image, register-staged (issued before the tile's products, written after)
// ------------------------------------------------------------------------------------------------
constexpr int FQ = 128, FK = 64;

// PAIR (causal, an even number of query blocks; profiles/r5zm_fpair): one workgroup runs query blocks
// nq - 1 - i and i one after the other, nq + 1 key tiles for every workgroup, half the grid.
// Measured and not taken: K / V tiles by LDS-DMA as the backward's (2-7 % slower,
// profiles/r5q_attn_split); 8 waves x 32 rows per workgroup (lost to attn_fwd_pp: profiles/r5zo_fwd8,
// profiles/r6d_attn_pp).
//
// The forwards' two MFMA phases with every LDS operand read RA MFMAs ahead of its use, the order
// pinned by sched groups (profiles/r6v_ra): the compiler's own order read each
// fragment one or two MFMAs early and waited on it there, so a wave paid an LDS round trip per
// k-step. S^T = K Q^T: MFMA i is k-step i / 2, key half t = i & 1.
template <int D, int RA>
__device__ __forceinline__ void qk_ra(const char* kimg, const int (&koff)[D / 16], const bf16x8 (&qf)[D / 16],
                                      f32x16 (&s)[2]) {
  constexpr int NM = D / 8;
  bf16x8 kf[NM];
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i == 0)
#pragma unroll
      for (int u = 0; u < RA; ++u) kf[u] = lds_row(kimg + 32 * (u & 1) * D * 2, koff[u >> 1]);
    if (i + RA < NM) kf[i + RA] = lds_row(kimg + 32 * ((i + RA) & 1) * D * 2, koff[(i + RA) >> 1]);
    s[i & 1] = mfma32(kf[i], qf[i >> 1], s[i & 1]);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, RA, 0);  // DS reads
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i + RA < NM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
  }
}

// O += P V: MFMA i is d tile n = i / 4, key half t = (i / 2) & 1, 16-key step s2 = i & 1, its A
// operand two transposed V reads
template <int D, int RA>
__device__ __forceinline__ void pv_ra(const char* vimg, const int (&voff0)[D / 32], const int (&voff1)[D / 32],
                                      const uint32_t (&pf)[2][2][4], f32x16 (&oa)[D / 32]) {
  constexpr int NM = D / 8;
  auto rd = [&](int i) __attribute__((always_inline)) {
    const char* base = vimg + (32 * ((i >> 1) & 1) + 16 * (i & 1)) * D * 2;
    return join(tr_read(base, voff0[i >> 2]), tr_read(base, voff1[i >> 2]));
  };
  bf16x8 vf[NM];
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i == 0)
#pragma unroll
      for (int u = 0; u < RA; ++u) vf[u] = rd(u);
    if (i + RA < NM) vf[i + RA] = rd(i + RA);
    const int t = (i >> 1) & 1, s2 = i & 1;
    const u32x4 pw = {pf[t][s2][0], pf[t][s2][1], pf[t][s2][2], pf[t][s2][3]};
    oa[i >> 2] = mfma32(vf[i], __builtin_bit_cast(bf16x8, pw), oa[i >> 2]);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, 2 * RA, 0);
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i + RA < NM) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  }
}

// attn_fwd (D = 64 and small grids): LDS reads pinned this many MFMAs ahead of their use (profiles/r6v_ra)
constexpr int kFwd4ReadAhead = 2;

template <int D, bool CAUSAL, bool PAIR = false>
__global__ __launch_bounds__(256, 2) void attn_fwd(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                   const __bf16* __restrict__ v, __bf16* __restrict__ o,
                                                   float* __restrict__ lse, AttnShape a) {
  constexpr int KS = D / 16;           // k-steps of the QK^T product
  constexpr int ND = D / 32;           // 32-wide d tiles of O
  constexpr int CH = D / 8;            // 16-B chunks per row
  constexpr int NT = 256, FQW = FQ;    // threads, query rows per workgroup (4 waves x 32)
  constexpr int NCH = FK * CH / NT;    // chunks per thread per K (and per V) tile
  constexpr int TILE = FK * D * 2;     // bytes of one K (or V) tile image
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];  // [buf][K, V]

  const int nq = (a.T + FQW - 1) / FQW;
  const BlockId bo = block_order(blockIdx.x, PAIR ? nq / 2 : nq, a.H * a.B, 64);  // workgroups per XCD
  const int bh = bo.bh, h = bh % a.H, b = bh / a.H;
#pragma unroll 1
  for (int pass = 0; pass < (PAIR ? 2 : 1); ++pass) {
  if (PAIR && pass) __syncthreads();  // the first block's last tile reads are done before the LDS is refilled
  const int qblk = pass ? bo.rank : nq - 1 - bo.rank;  // the heaviest (most keys) first

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int q0 = qblk * FQW, qw = q0 + 32 * w, qrow = qw + r;
  const int T = a.T;

  const __bf16* qb = q + base_off(a, TQ, b, h);
  const __bf16* kb = k + base_off(a, TK, b, h / a.G);  // grouped K / V heads: query head h reads head h / G
  const __bf16* vb = v + base_off(a, TV, b, h / a.G);
  const long long qt = a.s[TQ][2], kt = a.s[TK][2], vt = a.s[TV][2];

  bf16x8 qf[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    u32x4 x = {0u, 0u, 0u, 0u};
    if (qrow < T) x = gload16(qb + qrow * qt + kk * 16 + 8 * hh);
    qf[kk] = __builtin_bit_cast(bf16x8, x);
  }

  const int ntiles = CAUSAL ? min((T + FK - 1) / FK, (q0 + FQW) / FK) : (T + FK - 1) / FK;

  u32x4 kreg[NCH], vreg[NCH];
  const auto rk = slice_rsrc(kb, 2LL * T * kt), rv = slice_rsrc(vb, 2LL * T * vt);
  // The per-lane source offsets of the LDS-DMA staging that was measured and not taken (above). Nothing reads
  // them, but without them the compiler orders the staging loads of attn_fwd<128, *, false> and their registers
  // differently, and the kernel is then not the one that was measured: they stay until that is measured again.
  constexpr int NPC = TILE / 1024 / 4;
  const int wu = __builtin_amdgcn_readfirstlane(w);
  int dvo_k[NPC], dvo_v[NPC];
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const int byte = (wu * NPC + i) * 1024 + lane * 16;
    const int row = byte / (D * 2), ch = ((byte % (D * 2)) >> 4) ^ swz<D>(row, 0);
    dvo_k[i] = 2 * (row * (int)kt + ch * 8);
    dvo_v[i] = 2 * (row * (int)vt + ch * 8);
  }
  auto stage_load = [&](int tile) {
    const int k0 = tile * FK;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + NT * i, row = c / CH, ch = c % CH;
      // lane part in the voffset, the tile's row offset in the (scalar) soffset: no VALU per load
      kreg[i] = bload16(rk, 2 * (row * (int)kt + ch * 8), 2 * k0 * (int)kt);
      vreg[i] = bload16(rv, 2 * (row * (int)vt + ch * 8), 2 * k0 * (int)vt);
    }
  };
  auto stage_write = [&](int buf) {
    char* kimg = smem + buf * 2 * TILE;
    char* vimg = kimg + TILE;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + NT * i, row = c / CH, ch = c % CH;
      const int off = img_off<D>(row, ch);
      *reinterpret_cast<u32x4*>(kimg + off) = kreg[i];
      *reinterpret_cast<u32x4*>(vimg + off) = vreg[i];
    }
  };

  const float c = a.scale * kLog2e;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) oacc[n] = (f32x16){};

  stage_load(0);
  stage_write(0);
  __syncthreads();

  // per-lane LDS offsets of every operand read, computed once: the row parts that
  // vary per read (t, k-step, buffer) are compile-time and ride in the ds_read immediate, so the loop
  // body carries no address arithmetic (it was ~80 VALU per 64-key tile, a third of the VALU stream)
  int koff[KS], voff0[ND], voff1[ND];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) koff[kk] = img_off<D>(r, 2 * kk + hh);  // + 32 t rows: swz bits unchanged
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
    const int r0 = 4 * hh + qq;  // + kbase (a multiple of 16): swz bits unchanged
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int col = 32 * n + 16 * (g & 1) + 4 * pp;
      voff0[n] = img_off<D>(r0, col >> 3) + 8 * (pp & 1);
      voff1[n] = img_off<D>(r0 + 8, col >> 3) + 8 * (pp & 1);
    }
  }
  // the tile loop unrolled over the two buffers: the buffer offset is compile-time too
  auto tile_body = [&](int j, auto BUFC) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUFC)::value;
    const int k0 = j * FK;
    const bool more = j + 1 < ntiles;
    if (more) stage_load(j + 1);
    const char* kimg = smem + BUF * 2 * TILE;
    const char* vimg = kimg + TILE;
    // a wave whose 32 rows all precede the tile's first key has nothing to do (causal)
    if (!(CAUSAL && k0 > qw + 31)) {
      f32x16 sacc[2] = {(f32x16){}, (f32x16){}};
      qk_ra<D, kFwd4ReadAhead>(kimg, koff, qf, sacc);
      // masks: causal (key > query) on tiles that reach the wave's diagonal, key >= T on the tail
      const bool causal_mask = CAUSAL && k0 + FK - 1 > qw;
      if (causal_mask || k0 + FK > T) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = k0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
            if ((CAUSAL && key > qrow) || key >= T) sacc[t][e] = -INFINITY;
          }
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sacc[t][e]);
      mx = kfw::max_halves(mx);  // the row's other 32 keys (v_permlane32_swap; no LDS round trip)
      const float mn = fmaxf(m, mx);  // finite: the first tile holds key 0 <= every query
      // O and l are rescaled only when some row's max grew (exact: alpha == 1 otherwise); late in a
      // row's sweep that is the rare case, and the 64-register multiply is skipped
      const bool grew = __builtin_amdgcn_ballot_w64(mx > m) != 0;
      const float alpha = grew ? fast_exp2((m - mn) * c) : 1.f;
      m = mn;
      const float mc = mn * c;
      float rs = 0.f;
      uint32_t pf[2][2][4];  // [t][s][pair]: P^T as the B operand of PV
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const float p0 = fast_exp2(fmaf(sacc[t][e], c, -mc));
          const float p1 = fast_exp2(fmaf(sacc[t][e + 1], c, -mc));
          rs += p0 + p1;
          pf[t][e >> 3][(e & 7) >> 1] = pack2(p0, p1);
        }
      }
      if (grew) {
        l = l * alpha + rs;
#pragma unroll
        for (int n = 0; n < ND; ++n) oacc[n] *= alpha;
      } else {
        l += rs;
      }
      pv_ra<D, kFwd4ReadAhead>(vimg, voff0, voff1, pf, oacc);
    }
    if (more) stage_write(1 - BUF);
    __syncthreads();
  };
  for (int j = 0; j < ntiles; j += 2) {
    tile_body(j, std::integral_constant<int, 0>{});
    if (j + 1 < ntiles) tile_body(j + 1, std::integral_constant<int, 1>{});
  }

  // epilogue: lane (r, hh) holds row qrow, d = 32 n + (e & 3) + 8 (e >> 2) + 4 hh
  const float lt = kfw::sum_halves(l);
  const float inv = 1.f / lt;
  __bf16* ob = o + base_off(a, TO, b, h) + qrow * a.s[TO][2];
  store_rows16<ND>(ob, oacc, inv, qrow < T, hh);
  if (qrow < T && hh == 0) lse[((long long)b * a.H + h) * T + qrow] = m * a.scale + logf(lt);
  }  // pass
}

// ------------------------------------------------------------------------------------------------
// forward, 8 waves x 32 query rows = 256 rows per workgroup, one workgroup per CU
// (profiles/r6d_attn_pp): two waves per SIMD share its matrix pipe, one K / V image per CU per tile
// instead of two (half the LDS stores and global loads of attn_fwd's two 128-row workgroups), and the
// hardware interleaves one wave's softmax VALU with the other's MFMAs. One barrier per tile.
// The running max is a reference that moves only when a row's scores pass it by more than
// kFwdMaxThreshold (log2 units; cdna_hip_programming.md T13): probabilities stay <= 2^THR (exact in the
// fp32 l and O, bf16 keeps its relative precision), and the 64-register O rescale runs only on
// those tiles instead of on nearly every early one (the tests force both branches: rule 26).
// K / V are loaded two tiles ahead (a four-slot ring, two staging register sets).
// Measured and not taken (tools/attn_ab.py, profiles/r6d_attn_pp): staggering waves 4-7 half a tile
// behind waves 0-3 (MI355X_MICROARCH.md "Two waves per SIMD" item 9): +7 % time; the QK^T of tile
// j + 1 issued beside softmax(j), Q moved to LDS to pay for the second S tile (T15): +6 %; static
// priority 1 for waves 4-7, the second-dispatched half that loses every VALU arbitration to its SIMD
// partner (MI355X_MICROARCH.md "Two waves per SIMD" item 4); row max and row sum as 4 independent chains.
// ------------------------------------------------------------------------------------------------
// the running max moves only past this margin: probabilities stay <= 2^8, exact in fp32 l and O (profiles/r6d_attn_pp)
constexpr float kFwdMaxThreshold = 8.0f;
// attn_fwd_pp: LDS reads pinned this many MFMAs ahead of their use (profiles/r6v_ra)
constexpr int kFwdReadAhead = 2;
// scheduling fence between the QK^T / softmax / PV phases of attn_fwd_pp
#define FENCE() __builtin_amdgcn_sched_barrier(0)

template <int D, bool CAUSAL, bool PAIR>
__global__ __launch_bounds__(512, 1) void attn_fwd_pp(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                      const __bf16* __restrict__ v, __bf16* __restrict__ o,
                                                      float* __restrict__ lse, AttnShape a) {
  constexpr int KS = D / 16, ND = D / 32, CH = D / 8;
  constexpr int NT = 512, FQW = 256;
  constexpr int NCH = FK * CH / NT;  // 16-B chunks per thread per K (and per V) tile
  constexpr int TILE = FK * D * 2;
  // K ring [NS][TILE] then V ring [NS][TILE]; the V ring's base VBASE rides in the V read offsets,
  // so every slot / row offset of a read fits the 16-bit ds_read immediate
  constexpr int NS = 4, VBASE = NS * TILE;
  __shared__ __attribute__((aligned(16))) char smem[2 * NS * TILE];

  const int T = a.T;
  const int nq = (T + FQW - 1) / FQW, nta = (T + FK - 1) / FK;
  const BlockId bo = block_order(blockIdx.x, PAIR ? nq / 2 : nq, a.H * a.B, 32);  // one workgroup per CU
  const int bh = bo.bh, h = bh % a.H, b = bh / a.H;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int wu = __builtin_amdgcn_readfirstlane(w);  // the wave index as a uniform (scalar) value

  const __bf16* qb = q + base_off(a, TQ, b, h);
  const __bf16* kb = k + base_off(a, TK, b, h / a.G);  // grouped K / V heads: query head h reads head h / G
  const __bf16* vb = v + base_off(a, TV, b, h / a.G);
  const long long qt = a.s[TQ][2], kt = a.s[TK][2], vt = a.s[TV][2];
  const auto rk = slice_rsrc(kb, 2LL * T * kt), rv = slice_rsrc(vb, 2LL * T * vt);
  const float c = a.scale * kLog2e;
  constexpr float THR = kFwdMaxThreshold;

  // per-lane LDS offsets (as attn_fwd): tile row parts ride in the ds_read immediates
  int koff[KS], voff0[ND], voff1[ND];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) koff[kk] = img_off<D>(r, 2 * kk + hh);
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
    const int r0 = 4 * hh + qq;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int col = 32 * n + 16 * (g & 1) + 4 * pp;
      voff0[n] = VBASE + img_off<D>(r0, col >> 3) + 8 * (pp & 1);
      voff1[n] = VBASE + img_off<D>(r0 + 8, col >> 3) + 8 * (pp & 1);
    }
  }
  u32x4 kreg[NCH], vreg[NCH];
  auto qk = [&](const char* kimg, const bf16x8 (&qf)[KS], f32x16 (&s)[2]) __attribute__((always_inline)) {
    s[0] = (f32x16){};
    s[1] = (f32x16){};
    qk_ra<D, kFwdReadAhead>(kimg, koff, qf, s);
  };
  auto pv = [&](const char* vimg, const uint32_t (&pf)[2][2][4], f32x16 (&oa)[ND]) __attribute__((always_inline)) {
    pv_ra<D, kFwdReadAhead>(vimg, voff0, voff1, pf, oa);
  };
  // causal / tail mask of the wave's S^T tile (keys from k0, rows from qw); a uniform branch
  auto mask = [&](f32x16 (&s)[2], int k0, int qw) __attribute__((always_inline)) {
    if ((CAUSAL && k0 + FK - 1 > qw) || k0 + FK > T) {
      const int lim = (CAUSAL ? min(qw + r, T - 1) : T - 1) - k0 - 4 * hh;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (32 * t + (e & 3) + 8 * (e >> 2) > lim) s[t][e] = -INFINITY;
    }
  };
  // online softmax of one S^T tile into P (bf16 pairs: the PV B operand) and l; O is rescaled when
  // some lane's reference max moved
  auto softmax = [&](const f32x16 (&s)[2], float& m, float& l, uint32_t (&pf)[2][2][4], f32x16 (&oa)[ND])
                     __attribute__((always_inline)) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[t][e]);
    mx = kfw::max_halves(mx);
    const bool move = (mx - m) * c > THR;  // m = -inf on the first tile: moves
    const float mn = move ? mx : m;
    const float alpha = move ? fast_exp2((m - mn) * c) : 1.f;
    m = mn;
    const float mc = mn * c;
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const float p0 = fast_exp2(fmaf(s[t][e], c, -mc));
        const float p1 = fast_exp2(fmaf(s[t][e + 1], c, -mc));
        rs += p0 + p1;
        pf[t][e >> 3][(e & 7) >> 1] = pack2(p0, p1);
      }
    l = l * alpha + rs;
    if (__builtin_amdgcn_ballot_w64(move) != 0) {
#pragma unroll
      for (int n = 0; n < ND; ++n) oa[n] *= alpha;
    }
  };

  bf16x8 qf[KS];
  auto load_q = [&](int qr) __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      u32x4 x = {0u, 0u, 0u, 0u};
      if (qr < T) x = gload16(qb + qr * qt + kk * 16 + 8 * hh);
      qf[kk] = __builtin_bit_cast(bf16x8, x);
    }
  };
  // staging: two register sets, tile j + 2 issued at tile j (see the tile loop)
  u32x4 kr2[NCH], vr2[NCH];
  auto ld = [&](int tile, u32x4 (&kr)[NCH], u32x4 (&vr)[NCH]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cc = tid + NT * i, row = cc / CH, ch = cc % CH;
      kr[i] = bload16(rk, 2 * (row * (int)kt + ch * 8), 2 * tile * FK * (int)kt);
      vr[i] = bload16(rv, 2 * (row * (int)vt + ch * 8), 2 * tile * FK * (int)vt);
    }
  };
  auto st = [&](int slot, const u32x4 (&kr)[NCH], const u32x4 (&vr)[NCH]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cc = tid + NT * i;
      const int off = img_off<D>(cc / CH, cc % CH);
      *reinterpret_cast<u32x4*>(smem + slot * TILE + off) = kr[i];
      *reinterpret_cast<u32x4*>(smem + VBASE + slot * TILE + off) = vr[i];
    }
  };
  // pairs: the light block's Q and first two K / V tiles are issued when the heavy
  // block's tile loop ends, so their latency hides under its epilogue instead of stalling a second
  // prologue
  constexpr bool PXP = PAIR;

#pragma unroll 1
  for (int pass = 0; pass < (PAIR ? 2 : 1); ++pass) {
    if (PAIR && pass) __syncthreads();  // the first block's last reads are done before the LDS is refilled
    const int qblk = pass ? bo.rank : nq - 1 - bo.rank;  // the heaviest first
    const int q0 = qblk * FQW, qw = q0 + 32 * wu, qrow = qw + r;
    const int ntiles = CAUSAL ? min(nta, (q0 + FQW) / FK) : nta;
    const int jl = CAUSAL ? min(ntiles - 1, (qw + 31) / FK) : ntiles - 1;  // this wave's last tile
    const bool pre = PXP && pass == 1;  // Q and tiles 0 / 1 already in flight

    if (!pre) load_q(qrow);
    f32x16 oacc[ND], S[2][2];
#pragma unroll
    for (int n = 0; n < ND; ++n) oacc[n] = (f32x16){};
    float m = -INFINITY, l = 0.f;
    uint32_t pf[2][2][4];
    // tile j sits in ring slot j % 4, compile-time in the unrolled loop (pv reads through
    // smem + slot * TILE, the V ring base riding in voff)
    // K / V two tiles ahead: tile j + 2's loads are issued at tile j into the register set tile j
    // used (written at tile j - 1), and tile j + 1's set is written at the end of tile j into the
    // slot of tile j - 3 (a four-tile ring: slot and set compile-time in the 4x unrolled loop)
    if (!pre) ld(0, kreg, vreg);
    st(0, kreg, vreg);
    if (!pre && 1 < ntiles) ld(1, kr2, vr2);
    __syncthreads();
    auto tile = [&](int j, auto SLC) __attribute__((always_inline)) {
      constexpr int SL = decltype(SLC)::value;  // j % 4; register set j & 1
      auto& kc = (SL & 1) ? kr2 : kreg;
      auto& vc = (SL & 1) ? vr2 : vreg;
      auto& kn = (SL & 1) ? kreg : kr2;
      auto& vn = (SL & 1) ? vreg : vr2;
      if (j + 2 < ntiles) ld(j + 2, kc, vc);
      if (j <= jl) {
        qk(smem + SL * TILE, qf, S[0]);
        mask(S[0], j * FK, qw);
        FENCE();
        softmax(S[0], m, l, pf, oacc);
        FENCE();
        pv(smem + SL * TILE, pf, oacc);
      }
      if (j + 1 < ntiles) st((SL + 1) % 4, kn, vn);
      __syncthreads();
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    int j = 0;
#pragma unroll 1
    for (; j + 3 < ntiles; j += 4) {
      tile(j, I0{});
      tile(j + 1, I1{});
      tile(j + 2, I2{});
      tile(j + 3, I3{});
    }
    if (j < ntiles) tile(j, I0{});
    if (j + 1 < ntiles) tile(j + 1, I1{});
    if (j + 2 < ntiles) tile(j + 2, I2{});

    if (PXP && pass == 0) {  // the light block's Q and first K / V tiles, under this epilogue
      const int q0n = bo.rank * FQW;
      load_q(q0n + 32 * wu + r);
      ld(0, kreg, vreg);
      if (1 < (CAUSAL ? min(nta, (q0n + FQW) / FK) : nta)) ld(1, kr2, vr2);
    }

    // epilogue: lane (r, hh) holds row qrow, d = 32 n + (e & 3) + 8 (e >> 2) + 4 hh
    const float lt = kfw::sum_halves(l);
    const float inv = 1.f / lt;
    __bf16* ob = o + base_off(a, TO, b, h) + qrow * a.s[TO][2];
    store_rows16<ND>(ob, oacc, inv, qrow < T, hh);
    if (qrow < T && hh == 0) lse[((long long)b * a.H + h) * T + qrow] = m * a.scale + logf(lt);
  }  // pass
}

// ------------------------------------------------------------------------------------------------
// backward dQ without atomics: the forward's structure with the log-sum-exp known.
// One workgroup = 4 waves = 128 query rows; 64-key K / V tiles by LDS-DMA into a double-buffered
// image; per tile S^T = K Q^T and dP^T = V dO^T (keys on registers, the lane's query on the column),
// P^T = exp(scale S - lse), dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T with dS^T straight from the
// registers as the B operand (the permuted k order, as P^T feeds PV in the forward). dQ is written
// once, scaled, in bf16: no fp32 workspace, no atomics, no conversion pass. Costs the S and dP
// products a second time (the dK / dV kernel computes them too): against dQ by f32 atomics from the
// dK / dV kernel, gpt-1b 4x16x2048x128 bwd 570 -> 482 us, 16x12x2048x64 827 -> 557 (at D = 64 the
// atomics were a third of the pass), 1x16x4096x128 489 -> 417 (profiles/r5q_attn_split).
// This kernel runs first and is also the backward's prologue: each lane's query row computes
// delta = sum_d dO * O from the dO fragments it holds anyway plus one pass over O, and writes the two
// row constants of the dK / dV kernel in the form its products start from: nl = -lse / scale and
// nd = -delta (fp32 [B][H][T]); S - lse / scale and dP - delta are its MFMA accumulators initialised
// with nl and nd (no negate / scale per element and tile). Against a separate prologue kernel:
// gpt-1b bwd -5 %.
// PAIR: as attn_fwd's (query blocks nq - 1 - i and i in one workgroup). Measured twice and not taken
// (profiles/r5zm_fpair, profiles/r6v_ra), so only PAIR = false is instantiated; the pass loop stays
// because the compiler orders the kernel's prologue differently without it.
// Measured and not taken as well: LDS reads pinned ahead of their MFMAs as qk_ra / pv_ra (profiles/r6v_ra).
// ------------------------------------------------------------------------------------------------
template <int D, bool CAUSAL, bool PAIR = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_split(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                            const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ unused_slot,
                                                            __bf16* __restrict__ dq, AttnShape a,
                                                            const __bf16* __restrict__ o, float* __restrict__ nl_out,
                                                            float* __restrict__ nd_out) {
  constexpr int KS = D / 16;
  constexpr int ND = D / 32;
  constexpr int CH = D / 8;
  constexpr int TILE = FK * D * 2;             // one K (or V) tile image
  constexpr int NPC = TILE / 1024 / 4;         // LDS-DMA pieces (1 KiB) per wave per image
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];  // [buf][K, V]

  const int T = a.T;
  const int nq = (T + FQ - 1) / FQ;
  const BlockId bo = block_order(blockIdx.x, PAIR ? nq / 2 : nq, a.H * a.B, 64);
  const int bh = bo.bh, h = bh % a.H, b = bh / a.H;
#pragma unroll 1
  for (int pass = 0; pass < (PAIR ? 2 : 1); ++pass) {
  if (PAIR && pass) __syncthreads();  // the first block's last LDS reads are done before the refill
  const int qblk = pass ? bo.rank : nq - 1 - bo.rank;  // the heaviest first
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int q0 = qblk * FQ, qw = q0 + 32 * w, qrow = qw + r;

  const __bf16* qb = q + base_off(a, TQ, b, h);
  const __bf16* kb = k + base_off(a, TK, b, h / a.G);  // grouped K / V heads: query head h reads head h / G
  const __bf16* vb = v + base_off(a, TV, b, h / a.G);
  const __bf16* dob = dout + base_off(a, TDO, b, h);
  const long long qt = a.s[TQ][2], kt = a.s[TK][2], vt = a.s[TV][2], dot = a.s[TDO][2];
  const auto rq = slice_rsrc(qb, 2LL * T * qt), rdo = slice_rsrc(dob, 2LL * T * dot);
  const i32x4 dk_desc = slice_desc(kb, 2LL * T * kt), dv_desc = slice_desc(vb, 2LL * T * vt);

  // this lane's query: Q and dO rows as the B operands, lse and delta (rows past T: zeros)
  bf16x8 qf[KS], dof[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    qf[kk] = __builtin_bit_cast(bf16x8, bload16(rq, 2 * (qrow * (int)qt + kk * 16 + 8 * hh)));
    dof[kk] = __builtin_bit_cast(bf16x8, bload16(rdo, 2 * (qrow * (int)dot + kk * 16 + 8 * hh)));
  }
  const long long rowbase = ((long long)b * a.H + h) * T;
  const auto ro = slice_rsrc(o + base_off(a, TO, b, h), 2LL * T * a.s[TO][2]);
  float dd = 0.f;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const bf16x8 of = __builtin_bit_cast(bf16x8, bload16(ro, 2 * (qrow * (int)a.s[TO][2] + kk * 16 + 8 * hh)));
#pragma unroll
    for (int e = 0; e < 8; ++e) dd = fmaf((float)of[e], (float)dof[kk][e], dd);
  }
  const float delta_q = kfw::sum_halves(dd);  // the row's other half of d (lane ^ 32)
  const float lq = qrow < T ? lse[rowbase + qrow] : 0.f;
  const float nlc = -lq * kLog2e, nd_q = -delta_q;
  if (hh == 0 && qrow < T) {
    nl_out[rowbase + qrow] = -lq / a.scale;
    nd_out[rowbase + qrow] = nd_q;
  }

  const int ntiles = CAUSAL ? min((T + FK - 1) / FK, (q0 + FQ) / FK) : (T + FK - 1) / FK;
  // K / V tile `tile` -> image buffer `buf`, each lane fetching the chunk the swizzle puts at its slot
  // LDS-DMA pieces: the wave index as a uniform value, each piece's per-lane source offset computed
  // once (image chunk sc of row `row` holds source chunk sc ^ swz(row, 0))
  const int wu = __builtin_amdgcn_readfirstlane(w);
  int dvo_k[NPC], dvo_v[NPC];
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const int byte = (wu * NPC + i) * 1024 + lane * 16;
    const int row = byte / (D * 2), ch = ((byte % (D * 2)) >> 4) ^ swz<D>(row, 0);
    dvo_k[i] = 2 * (row * (int)kt + ch * 8);
    dvo_v[i] = 2 * (row * (int)vt + ch * 8);
  }
  auto stage_dma = [&](int tile, int buf) {
    const int k0 = tile * FK;
    char* kimg = smem + buf * 2 * TILE;
    char* vimg = kimg + TILE;
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      dma16(dk_desc, lds_addr(kimg + (wu * NPC + i) * 1024), dvo_k[i], 2 * k0 * (int)kt);
      dma16(dv_desc, lds_addr(vimg + (wu * NPC + i) * 1024), dvo_v[i], 2 * k0 * (int)vt);
    }
  };

  const float c = a.scale * kLog2e;
  f32x16 dqacc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) dqacc[n] = (f32x16){};

  if (ntiles > 0) stage_dma(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // per-lane LDS read offsets computed once; the tile loop unrolled over the two buffers (as the forward)
  int koff[KS], voff0[ND], voff1[ND];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) koff[kk] = img_off<D>(r, 2 * kk + hh);
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int col = 32 * n + 16 * (g & 1) + 4 * pp;
      voff0[n] = img_off<D>(4 * hh + qq, col >> 3) + 8 * (pp & 1);
      voff1[n] = img_off<D>(4 * hh + qq + 8, col >> 3) + 8 * (pp & 1);
    }
  }
  auto tile_body = [&](int j, auto BUFC) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUFC)::value;
    const int k0 = j * FK;
    if (j + 1 < ntiles) stage_dma(j + 1, 1 - BUF);  // buffer 1 - BUF was last read before the barrier
    const char* kimg = smem + BUF * 2 * TILE;
    const char* vimg = kimg + TILE;
    if (!(CAUSAL && k0 > qw + 31)) {
      f32x16 sacc[2] = {(f32x16){}, (f32x16){}}, dpacc[2] = {(f32x16){}, (f32x16){}};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          sacc[t] = mfma32(lds_row(kimg + 32 * t * D * 2, koff[kk]), qf[kk], sacc[t]);
          dpacc[t] = mfma32(lds_row(vimg + 32 * t * D * 2, koff[kk]), dof[kk], dpacc[t]);
        }
      }
      const bool need_mask = (CAUSAL && k0 + FK - 1 > qw) || k0 + FK > T;
      uint32_t sf[2][2][4];  // [t][s][pair]: dS^T as the B operand of K^T dS^T
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          float p0 = fast_exp2(fmaf(sacc[t][e], c, nlc)), p1 = fast_exp2(fmaf(sacc[t][e + 1], c, nlc));
          if (need_mask) {
            const int key = k0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
            if ((CAUSAL && key > qrow) || key >= T) p0 = 0.f;
            if ((CAUSAL && key + 1 > qrow) || key + 1 >= T) p1 = 0.f;
          }
          sf[t][e >> 3][(e & 7) >> 1] = pack2(p0 * (dpacc[t][e] + nd_q), p1 * (dpacc[t][e + 1] + nd_q));
        }
      }
#pragma unroll
      for (int n = 0; n < ND; ++n) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 kf = join(tr_read(kimg + (32 * t + 16 * s2) * D * 2, voff0[n]),
                                   tr_read(kimg + (32 * t + 16 * s2) * D * 2, voff1[n]));
            const u32x4 sw = {sf[t][s2][0], sf[t][s2][1], sf[t][s2][2], sf[t][s2][3]};
            dqacc[n] = mfma32(kf, __builtin_bit_cast(bf16x8, sw), dqacc[n]);
          }
        }
      }
    }
    // the next tile's pieces (the only vector-memory operations in the loop) have landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  for (int j = 0; j < ntiles; j += 2) {
    tile_body(j, std::integral_constant<int, 0>{});
    if (j + 1 < ntiles) tile_body(j + 1, std::integral_constant<int, 1>{});
  }

  // lane (r, hh) holds row qrow, d = 32 n + (e & 3) + 8 (e >> 2) + 4 hh
  __bf16* dqr = dq + base_off(a, TDQ, b, h) + qrow * a.s[TDQ][2];
  store_rows16<ND>(dqr, dqacc, a.scale, qrow < T, hh);
  }  // pass
}

// ------------------------------------------------------------------------------------------------
// backward dK / dV: one workgroup = 128 keys of one (b, h); 64-row query tiles (Q, dO, nl, nd, as
// attn_bwd_dq_split wrote them) double-buffered through LDS by LDS-DMA; dK / dV in registers for the
// whole sweep. Two waves per SIMD: 8 waves = 4 key
// groups of 32 keys x 2 query halves. Wave (w, jh) takes rows 32 jh .. 32 jh + 31 of every 64-row
// query tile for the keys of group w, so the two waves of a SIMD interleave their LDS waits and
// barriers with each other's MFMAs (with 4 waves, one per SIMD at D = 128, a wave waited half its
// cycles: profiles/r5w_attn_dkdv8; D = 64, 16x12x2048x64: 516 -> 485 us). K and V both sit in LDS
// (V rows are the dP product's B operand) to keep a wave
// within 256 registers; the two halves' partial dK^T / dV^T are summed through LDS at the end.
//
// GRP (grouped-query attention, Hkv < H): the grid runs over K / V heads, nk * Hkv * B * (G / GS)
// workgroups. A workgroup keeps its 128 keys' dK^T / dV^T in registers as above and sweeps the query
// tiles of GS query heads of the group, head after head, as ONE flat tile sequence: the double buffer
// keeps running across a head boundary, only the Q / dO / nl / nd descriptors of the staged tile switch
// (SGPR quads rebuilt per staged tile: a few scalar instructions). GS = G: the group's sum is complete
// in fp32 registers, rounded once and stored as bf16 with Hkv heads. GS < G: the G / GS workgroups
// ("parts") of a (key block, K / V head) store their unscaled fp32 sums to `gpart`
// ([dk, dv][part][B][Hkv][T][D]) and attn_bwd_gqa_reduce adds the parts in part order, scales, rounds
// once and stores: no atomics on either route, both deterministic. GRP = false: one query head per K / V head.
// Registers (hipcc 7.2 remarks; no scratch anywhere): D = 128 causal / full 226 / 222 VGPRs ungrouped,
// 227 / 228 GRP; D = 64 126 / 128 ungrouped, 124 / 128 GRP. GRP at D = 64 asks for 4 waves per SIMD
// in its launch bounds: unforced, the non-causal kernel took 142 VGPRs and lost the second workgroup per CU.
// ------------------------------------------------------------------------------------------------
constexpr int BK = 128, BQ = 64;

template <int D, bool CAUSAL, bool GRP = false>
__global__ __launch_bounds__(512, D == 64 ? (GRP ? 4 : 2) : 1) void attn_bwd_dkdv8(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                         const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                         const float* __restrict__ nl, const float* __restrict__ nd,
                                                         __bf16* __restrict__ dk, __bf16* __restrict__ dv, AttnShape a,
                                                         float* __restrict__ gpart) {
  constexpr int KS = D / 16;
  constexpr int ND = D / 32;
  constexpr int CH = D / 8;
  constexpr int KIMG = BK * D * 2;          // K (and V) image: [128 keys][D]
  constexpr int QT = BQ * D * 2;            // one Q (or dO) tile image: [64][D]
  constexpr int NPC = QT / 1024 / 8;        // LDS-DMA pieces per wave per tile image
  static_assert(NPC >= 1, "head dim");
  static_assert(4 * QT >= 4 * ND * 4 * 1024, "partial-sum staging fits the Q / dO region");
  __shared__ __attribute__((aligned(16))) char smem[2 * KIMG + 4 * QT + 4 * BQ * 4];
  char* const kimg = smem;
  char* const vimg = smem + KIMG;
  char* const qtiles = smem + 2 * KIMG;     // [buf][Q, dO]
  float* const rowc = reinterpret_cast<float*>(qtiles + 4 * QT);  // [buf][nl(64), nd(64)]

  const int T = a.T;
  const int nk = (T + BK - 1) / BK;
  // GRP: the part (which GS query heads of the group) outermost, so that with a grid per part that is a
  // multiple of 8 the parts of one K / V head land on the same XCD (its K / V tiles in one L2)
  const int HK = GRP ? a.Hkv : a.H;  // heads the grid runs over
  const int nkv = nk * HK * a.B;
  const int gp = GRP ? blockIdx.x / nkv : 0;
  const BlockId bo = block_order(GRP ? blockIdx.x - gp * nkv : blockIdx.x, nk, HK * a.B, D == 64 ? 64 : 32);
  const int kblk = bo.rank;  // block 0 (all queries) first
  const int bh = bo.bh, hk = bh % HK, b = bh / HK;  // hk: the head of K, V, dK, dV
  const int h = GRP ? hk * a.G + gp * a.GS : hk;  // (the first of) this workgroup's query head(s)
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7, uniform
  const int w = wv & 3, jh = wv >> 2;                       // key group, query half
  const int k0 = kblk * BK, kw = k0 + 32 * w, key = kw + r;

  const __bf16* qb = q + base_off(a, TQ, b, h);
  const __bf16* kb = k + base_off(a, TK, b, hk);
  const __bf16* vb = v + base_off(a, TV, b, hk);
  const __bf16* dob = dout + base_off(a, TDO, b, h);
  const long long qt = a.s[TQ][2], kt = a.s[TK][2], vt = a.s[TV][2], dot = a.s[TDO][2];
  const float* nlb = nl + ((long long)b * a.H + h) * T;
  const float* ndb = nd + ((long long)b * a.H + h) * T;
  const auto rk = slice_rsrc(kb, 2LL * T * kt), rv = slice_rsrc(vb, 2LL * T * vt);

  // K and V images of the block's 128 keys (rows past T: zeros)
#pragma unroll
  for (int i = 0; i < BK * CH / 512; ++i) {
    const int c = tid + 512 * i, row = c / CH, ch = c % CH;
    *reinterpret_cast<u32x4*>(kimg + img_off<D>(row, ch)) = bload16(rk, 2 * (row * (int)kt + ch * 8), 2 * k0 * (int)kt);
    *reinterpret_cast<u32x4*>(vimg + img_off<D>(row, ch)) = bload16(rv, 2 * (row * (int)vt + ch * 8), 2 * k0 * (int)vt);
  }

  const int qstart = CAUSAL ? k0 : 0;
  const int ntiles = (T - qstart + BQ - 1) / BQ;

  const i32x4 dq_desc = slice_desc(qb, 2LL * T * qt), ddo_desc = slice_desc(dob, 2LL * T * dot);
  const i32x4 drow_desc = slice_desc(wv == 0 ? nlb : ndb, 4LL * T);
  int dvo_q[NPC], dvo_o[NPC];
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const int byte = (wv * NPC + i) * 1024 + lane * 16;
    const int row = byte / (D * 2), ch = ((byte % (D * 2)) >> 4) ^ swz<D>(row, 0);
    dvo_q[i] = 2 * (row * (int)qt + ch * 8);
    dvo_o[i] = 2 * (row * (int)dot + ch * 8);
  }
  // g (GRP): the tile's query head within this workgroup's GS heads: Q, dO, nl, nd of head h + g
  auto stage_dma = [&](int tile, int buf, int g = 0) {
    const int q0 = qstart + tile * BQ;
    char* qi = qtiles + buf * 2 * QT;
    char* oi = qi + QT;
    const i32x4 dq_d = GRP ? slice_desc(qb + g * a.s[TQ][1], 2LL * T * qt) : dq_desc;
    const i32x4 ddo_d = GRP ? slice_desc(dob + g * a.s[TDO][1], 2LL * T * dot) : ddo_desc;
    const i32x4 drow_d = GRP ? slice_desc((wv == 0 ? nlb : ndb) + (long long)g * T, 4LL * T) : drow_desc;
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      dma16(dq_d, lds_addr(qi + (wv * NPC + i) * 1024), dvo_q[i], 2 * q0 * (int)qt);
      dma16(ddo_d, lds_addr(oi + (wv * NPC + i) * 1024), dvo_o[i], 2 * q0 * (int)dot);
    }
    if (wv < 2) dma4(drow_d, lds_addr(reinterpret_cast<const char*>(rowc + buf * 2 * BQ + wv * BQ)), 4 * lane, 4 * q0);
  };
  // GRP: the flat sequence of GS * ntiles tiles; (sg, st) = the head and tile that the next staging loads
  const int nflat = (GRP ? a.GS : 1) * ntiles;
  int sg = 0, st = 0;
  auto stage_next = [&](int buf) {
    stage_dma(st, buf, sg);
    if (++st == ntiles) {
      st = 0;
      ++sg;
    }
  };

  int koff[KS], voff0[ND], voff1[ND];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) koff[kk] = img_off<D>(r, 2 * kk + hh);
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int col = 32 * n + 16 * (g & 1) + 4 * pp;
      voff0[n] = img_off<D>(4 * hh + qq, col >> 3) + 8 * (pp & 1);
      voff1[n] = img_off<D>(4 * hh + qq + 8, col >> 3) + 8 * (pp & 1);
    }
  }
  const char* const kimg_w = kimg + 32 * w * D * 2;
  const char* const vimg_w = vimg + 32 * w * D * 2;

  const float c = a.scale * kLog2e;
  f32x16 dkacc[ND], dvacc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) {
    dkacc[n] = (f32x16){};
    dvacc[n] = (f32x16){};
  }

  if (ntiles > 0) {
    if constexpr (GRP) stage_next(0);
    else stage_dma(0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // it: the tile's index within its head's sweep; more: another tile follows (GRP: maybe of the next head)
  auto tile_body = [&](int it, bool more, auto BUFC) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUFC)::value;
    const int q0 = qstart + it * BQ;
    if (more) {
      if constexpr (GRP) stage_next(1 - BUF);
      else stage_dma(it + 1, 1 - BUF);
    }
    const char* qi = qtiles + BUF * 2 * QT + 32 * jh * D * 2;  // this wave's 32 query rows
    const char* oi = qi + QT;
    const float* nl_s = rowc + BUF * 2 * BQ + 32 * jh;
    const float* nd_s = nl_s + BQ;
    const int qw = q0 + 32 * jh;
    // causal: every query of the half precedes every key of the wave -> P = dS = 0
    if (!(CAUSAL && qw + 31 < kw)) {
      const bool need_mask = (CAUSAL && qw < kw + 31) || qw + 32 > T || key >= T;
      f32x16 sacc, dpacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(nl_s + 8 * g + 4 * hh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(nd_s + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sacc[4 * g + e] = l4[e];
          dpacc[4 * g + e] = d4[e];
        }
      }
      // rows = this wave's queries, column = the lane's key
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        sacc = mfma32(lds_row(qi, koff[kk]), lds_row(kimg_w, koff[kk]), sacc);
        dpacc = mfma32(lds_row(oi, koff[kk]), lds_row(vimg_w, koff[kk]), dpacc);
      }
      uint32_t pf[2][4], sf[2][4];
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        float p0 = fast_exp2(sacc[e] * c), p1 = fast_exp2(sacc[e + 1] * c);
        if (need_mask) {
          const int qa0 = qw + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if ((CAUSAL && qa0 < key) || qa0 >= T || key >= T) p0 = 0.f;
          if ((CAUSAL && qa0 + 1 < key) || qa0 + 1 >= T || key >= T) p1 = 0.f;
        }
        pf[e >> 3][(e & 7) >> 1] = pack2(p0, p1);
        sf[e >> 3][(e & 7) >> 1] = pack2(p0 * dpacc[e], p1 * dpacc[e + 1]);
      }
      // dV^T += dO^T . P and dK^T += Q^T . dS over this half's rows (permuted k order)
#pragma unroll
      for (int n = 0; n < ND; ++n) {
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
          const u32x4 pw = {pf[sx][0], pf[sx][1], pf[sx][2], pf[sx][3]};
          const u32x4 sw = {sf[sx][0], sf[sx][1], sf[sx][2], sf[sx][3]};
          const bf16x8 doa = join(tr_read(oi + 16 * sx * D * 2, voff0[n]), tr_read(oi + 16 * sx * D * 2, voff1[n]));
          dvacc[n] = mfma32(doa, __builtin_bit_cast(bf16x8, pw), dvacc[n]);
          const bf16x8 qa = join(tr_read(qi + 16 * sx * D * 2, voff0[n]), tr_read(qi + 16 * sx * D * 2, voff1[n]));
          dkacc[n] = mfma32(qa, __builtin_bit_cast(bf16x8, sw), dkacc[n]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile's pieces (the loop's only VMEM)
    __syncthreads();
  };
  if constexpr (GRP) {
    int ct = 0;  // the computed tile's index within its head
    for (int f = 0; f < nflat; f += 2) {
      tile_body(ct, f + 1 < nflat, std::integral_constant<int, 0>{});
      if (++ct == ntiles) ct = 0;
      if (f + 1 < nflat) {
        tile_body(ct, f + 2 < nflat, std::integral_constant<int, 1>{});
        if (++ct == ntiles) ct = 0;
      }
    }
  } else {
    for (int it = 0; it < ntiles; it += 2) {
      tile_body(it, it + 1 < ntiles, std::integral_constant<int, 0>{});
      if (it + 1 < ntiles) tile_body(it + 1, it + 2 < ntiles, std::integral_constant<int, 1>{});
    }
  }

  // the two query halves' partial sums: half 1 stages its accumulators (f32, lane-major) in the
  // Q / dO region, half 0 adds them and stores; dK first, then dV
  float* const part = reinterpret_cast<float*>(qtiles);
  auto reduce = [&](f32x16 (&acc)[ND]) __attribute__((always_inline)) {
    if (jh == 1) {
#pragma unroll
      for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(part + (((w * ND + n) * 4 + g) * 64 + lane) * 4) =
              (f32x4){acc[n][4 * g], acc[n][4 * g + 1], acc[n][4 * g + 2], acc[n][4 * g + 3]};
    }
    __syncthreads();
    if (jh == 0) {
#pragma unroll
      for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(part + (((w * ND + n) * 4 + g) * 64 + lane) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[n][4 * g + e] += x[e];
        }
    }
    __syncthreads();
  };
  reduce(dkacc);
  reduce(dvacc);
  // lane = key, rows d = 32 n + (e & 3) + 8 (e >> 2) + 4 hh
  if constexpr (GRP) {
    if (a.GS != a.G) {  // this part's unscaled fp32 sums, [dk, dv][part][B][Hkv][T][D]: attn_bwd_gqa_reduce finishes
      if (jh == 0 && key < T) {
        const long long per = (long long)a.B * a.Hkv * T * D;  // one part of one tensor
        float* pk = gpart + gp * per + (((long long)b * a.Hkv + hk) * T + key) * D;
        float* pv = pk + (a.G / a.GS) * per;
#pragma unroll
        for (int n = 0; n < ND; ++n) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int d = 32 * n + 8 * g + 4 * hh;
            *reinterpret_cast<f32x4*>(pk + d) = (f32x4){dkacc[n][4 * g], dkacc[n][4 * g + 1], dkacc[n][4 * g + 2], dkacc[n][4 * g + 3]};
            *reinterpret_cast<f32x4*>(pv + d) = (f32x4){dvacc[n][4 * g], dvacc[n][4 * g + 1], dvacc[n][4 * g + 2], dvacc[n][4 * g + 3]};
          }
        }
      }
      return;
    }
  }
  if (jh == 0) {  // (jh: wave-uniform, so whole waves run the swaps)
    store_rows16<ND>(dk + base_off(a, TDK, b, hk) + key * a.s[TDK][2], dkacc, a.scale, key < T, hh);
    store_rows16<ND>(dv + base_off(a, TDV, b, hk) + key * a.s[TDV][2], dvacc, 1.f, key < T, hh);
  }
}

// The group-split route's second pass (attn_bwd_dkdv8 GRP with GS < G): dk / dv (bf16, strided, Hkv heads) =
// the NP = G / GS fp32 parts of a row added in part order (fixed: bit-identical from call to call), dk scaled,
// each rounded once. One thread per 8 columns of one (b, hkv, t) row, both tensors.
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_gqa_reduce(const float* __restrict__ gpart, __bf16* __restrict__ dk,
                                                           __bf16* __restrict__ dv, AttnShape a) {
  constexpr int LPR = D / 8;
  constexpr int RPB = 256 / LPR;
  const long long nrows = (long long)a.B * a.Hkv * a.T;
  const long long row = (long long)blockIdx.x * RPB + threadIdx.x / LPR;
  const int c8 = threadIdx.x % LPR;
  if (row >= nrows) return;
  const int t = (int)(row % a.T);
  const int hk = (int)((row / a.T) % a.Hkv);
  const int b = (int)(row / ((long long)a.T * a.Hkv));
  const int np = a.G / a.GS;
  const long long per = nrows * D;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const float* src = gpart + which * np * per + row * D + c8 * 8;
    f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
    for (int p = 1; p < np; ++p) {
      src += per;
      const f32x4 y0 = *reinterpret_cast<const f32x4*>(src), y1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x0[e] += y0[e];
        x1[e] += y1[e];
      }
    }
    const float s = which == 0 ? a.scale : 1.f;
    const u32x4 y = {pack2(x0[0] * s, x0[1] * s), pack2(x0[2] * s, x0[3] * s), pack2(x1[0] * s, x1[1] * s),
                     pack2(x1[2] * s, x1[3] * s)};
    __bf16* dst = which == 0 ? dk + base_off(a, TDK, b, hk) + t * a.s[TDK][2] : dv + base_off(a, TDV, b, hk) + t * a.s[TDV][2];
    *reinterpret_cast<u32x4*>(dst + c8 * 8) = y;
  }
}

bool fill_shape(AttnShape& s, int B, int H, int T, int D, float scale, const long long* strides, int ntensors) {
  if (B <= 0 || H <= 0 || T <= 0 || (D != 64 && D != 128) || !strides) return false;
  s.B = B;
  s.H = H;
  s.T = T;
  s.scale = scale;
  s.Hkv = H;
  s.G = s.GS = 1;
  for (int t = 0; t < 8; ++t)
    for (int j = 0; j < 3; ++j) s.s[t][j] = t < ntensors ? strides[3 * t + j] : 0;
  for (int t = 0; t < ntensors; ++t)
    for (int j = 0; j < 3; ++j)
      if (strides[3 * t + j] & 7) return false;  // 16-B aligned rows
  return true;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// compute units of the current device, queried once (256 on MI355X)
int device_cus() {
  static const int n = [] {
    int cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      cus = 256;
    return cus > 0 ? cus : 256;
  }();
  return n;
}

// a (b, h) slice of T rows read through a buffer descriptor: 32-bit byte offsets
bool slice_ok(int T, long long row_stride, int elem_bytes) {
  return row_stride > 0 && (long long)T * row_stride * elem_bytes < (1ll << 31);
}

// Hkv K / V heads for H query heads: at least one, dividing H
bool set_kv_heads(AttnShape& s, int Hkv) {
  if (Hkv < 1 || s.H % Hkv != 0) return false;
  s.Hkv = Hkv;
  s.G = s.H / Hkv;
  s.GS = s.G;
  return true;
}

// The dK / dV group split (attn_bwd_dkdv8 GRP): GS query heads of a group per workgroup. Sweeping the whole
// group (GS = G) shrinks the grid by G (B = 1, Hkv = 2, T = 2048: 32 workgroups on 256 CUs), and a causal grid
// that only just fills the chip finishes with its heaviest workgroup (key block 0: GS times every query tile).
// So: the largest divisor GS of G whose grid nk * Hkv * B * (G / GS) has at least 1.5 workgroups per slot
// (slots = compute units x resident workgroups: 1 at D = 128, 2 at D = 64), else 1 (every query head its own
// workgroup, as the ungrouped kernel, plus the reduce pass). Measured (profiles/flash_gqa, causal T = 2048,
// medians of 7 interleaved blocks, us; * = this rule's pick, within the spread of the best everywhere):
//   4x16 D=128  G=2: GS 2 254* 1 302 | G=4: GS 4 317, 2 268*, 1 300 | G=8: GS 8 503, 4 326, 2 315*, 1 314
//   16x12 D=64  G=2: GS 2 423* 1 473 | G=4: GS 4 401*, 2 431, 1 465 | G=6: GS 6 449, 3 422*, 2 456, 1 468
//   1x8 D=128   G=4: GS 4 261, 2 169, 1 125*
// (the first rule, one workgroup per compute unit, picked GS = 4 at 4x16 G = 4 and 8, and GS = 6 at 16x12 G = 6).
int gqa_group_split(int B, int H, int Hkv, int T, int D) {
  const int G = H / Hkv;
  const long long nkv = (long long)((T + BK - 1) / BK) * Hkv * B;
  const long long slots = (long long)device_cus() * (D == 64 ? 2 : 1);
  for (int gs = G; gs > 1; --gs)
    if (G % gs == 0 && 2 * nkv * (G / gs) >= 3 * slots) return gs;
  return 1;
}

long long align16(long long n) { return (n + 15) & ~15ll; }

int attn_fwd_launch(const void* q, const void* k, const void* v, void* o, void* lse, int B, int H, int Hkv, int T,
                    int D, float scale, int causal, const long long* strides, void* stream) {
  AttnShape s;
  if (!q || !k || !v || !o || !lse) return KFAMD_EINVAL;
  if (!fill_shape(s, B, H, T, D, scale, strides, 4) || !set_kv_heads(s, Hkv)) return KFAMD_EINVAL;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(o)) return KFAMD_EALIGN;
  const long long nwg = (long long)((T + FQ - 1) / FQ) * H * B;
  if (nwg >= (1ll << 31)) return KFAMD_EINVAL;
  if (!slice_ok(T, s.s[TK][2], 2) || !slice_ok(T, s.s[TV][2], 2)) return KFAMD_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), 0, st, static_cast<const __bf16*>(q),
                       static_cast<const __bf16*>(k), static_cast<const __bf16*>(v), static_cast<__bf16*>(o),
                       static_cast<float*>(lse), s);
  };
  const int nq = (T + FQ - 1) / FQ;
  const int nq4 = (T + 255) / 256;
  const bool pair4 = causal && nq4 % 2 == 0;
  const long long g4 = (long long)(pair4 ? nq4 / 2 : nq4) * H * B;
  // attn_fwd_pp where its grid fills the chip (one workgroup per CU); attn_fwd otherwise and at
  // D = 64, where the two-workgroups-per-CU kernel measured faster (profiles/r6d_attn_pp)
  if (D == 128 && g4 >= device_cus()) {
    const bool pair = pair4;
    auto go4 = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((unsigned)g4), dim3(512), 0, st, static_cast<const __bf16*>(q),
                         static_cast<const __bf16*>(k), static_cast<const __bf16*>(v), static_cast<__bf16*>(o),
                         static_cast<float*>(lse), s);
    };
    pair ? go4(attn_fwd_pp<128, true, true>) : causal ? go4(attn_fwd_pp<128, true, false>)
                                                   : go4(attn_fwd_pp<128, false, false>);
  } else if (causal && nq % 2 == 0) {
    auto go2 = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((unsigned)(nwg / 2)), dim3(256), 0, st, static_cast<const __bf16*>(q),
                         static_cast<const __bf16*>(k), static_cast<const __bf16*>(v), static_cast<__bf16*>(o),
                         static_cast<float*>(lse), s);
    };
    if (D == 128) go2(attn_fwd<128, true, true>);
    else go2(attn_fwd<64, true, true>);
  } else if (D == 128) {
    causal ? go(attn_fwd<128, true>) : go(attn_fwd<128, false>);
  } else {
    causal ? go(attn_fwd<64, true>) : go(attn_fwd<64, false>);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

// One schedule: attn_bwd_dq_split (dQ, and the row constants nl / nd into the workspace), then attn_bwd_dkdv8,
// then (grouped K / V with GS < G) attn_bwd_gqa_reduce over the parts' fp32 sums behind nl / nd in the workspace.
// group_split: 0 = gqa_group_split's rule, else the GS to use (a divisor of G). Hkv == H: the ungrouped kernels.
int attn_bwd_launch(const void* q, const void* k, const void* v, const void* o, const void* dout, const void* lse,
                    void* dq, void* dk, void* dv, void* workspace, int B, int H, int Hkv, int T, int D, float scale,
                    int causal, int group_split, const long long* strides, void* stream) {
  AttnShape s;
  if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv || !workspace) return KFAMD_EINVAL;
  if (!fill_shape(s, B, H, T, D, scale, strides, 8) || !set_kv_heads(s, Hkv)) return KFAMD_EINVAL;
  if (group_split < 0 || (group_split > 0 && s.G % group_split != 0)) return KFAMD_EINVAL;
  const bool grouped = Hkv != H;
  if (grouped) s.GS = group_split > 0 ? group_split : gqa_group_split(B, H, Hkv, T, D);
  if (!al16(q) || !al16(k) || !al16(v) || !al16(o) || !al16(dout) || !al16(dq) || !al16(dk) || !al16(dv) ||
      !al16(workspace))
    return KFAMD_EALIGN;
  const long long nk = (long long)((T + BK - 1) / BK) * H * B;
  if (nk >= (1ll << 31)) return KFAMD_EINVAL;
  if (!slice_ok(T, s.s[TQ][2], 2) || !slice_ok(T, s.s[TDO][2], 2)) return KFAMD_EINVAL;
  if (!slice_ok(T, s.s[TK][2], 2) || !slice_ok(T, s.s[TV][2], 2)) return KFAMD_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* nl = static_cast<float*>(workspace);  // -lse / scale and -delta, [B][H][T] each
  float* nd = nl + (long long)B * H * T;
  const long long nq = (long long)((T + FQ - 1) / FQ) * H * B;
  // grouped K / V: the dK / dV grid runs over K / V heads and the G / GS parts of each group
  const long long nkg = grouped ? nk / s.G * (s.G / s.GS) : nk;
  float* gpart = grouped && s.GS != s.G ? reinterpret_cast<float*>(static_cast<char*>(workspace) + align16(2LL * B * H * T * 4))
                                        : nullptr;
  auto run = [&](auto dq_k, auto dkdv_k, auto reduce_k) {
    hipLaunchKernelGGL(dq_k, dim3((unsigned)nq), dim3(256), 0, st, static_cast<const __bf16*>(q),
                       static_cast<const __bf16*>(k), static_cast<const __bf16*>(v), static_cast<const __bf16*>(dout),
                       static_cast<const float*>(lse), static_cast<const float*>(nullptr), static_cast<__bf16*>(dq), s,
                       static_cast<const __bf16*>(o), nl, nd);
    hipLaunchKernelGGL(dkdv_k, dim3((unsigned)nkg), dim3(512), 0, st, static_cast<const __bf16*>(q),
                       static_cast<const __bf16*>(k), static_cast<const __bf16*>(v), static_cast<const __bf16*>(dout),
                       static_cast<const float*>(nl), static_cast<const float*>(nd), static_cast<__bf16*>(dk),
                       static_cast<__bf16*>(dv), s, gpart);
    if (gpart) {
      const long long krows = (long long)B * Hkv * T;
      const unsigned kblocks = (unsigned)((krows + 256 / (D / 8) - 1) / (256 / (D / 8)));
      hipLaunchKernelGGL(reduce_k, dim3(kblocks), dim3(256), 0, st, gpart, static_cast<__bf16*>(dk),
                         static_cast<__bf16*>(dv), s);
    }
  };
  if (D == 128) {
    if (grouped) causal ? run(attn_bwd_dq_split<128, true>, attn_bwd_dkdv8<128, true, true>, attn_bwd_gqa_reduce<128>)
                        : run(attn_bwd_dq_split<128, false>, attn_bwd_dkdv8<128, false, true>, attn_bwd_gqa_reduce<128>);
    else causal ? run(attn_bwd_dq_split<128, true>, attn_bwd_dkdv8<128, true>, attn_bwd_gqa_reduce<128>)
                : run(attn_bwd_dq_split<128, false>, attn_bwd_dkdv8<128, false>, attn_bwd_gqa_reduce<128>);
  } else {
    if (grouped) causal ? run(attn_bwd_dq_split<64, true>, attn_bwd_dkdv8<64, true, true>, attn_bwd_gqa_reduce<64>)
                        : run(attn_bwd_dq_split<64, false>, attn_bwd_dkdv8<64, false, true>, attn_bwd_gqa_reduce<64>);
    else causal ? run(attn_bwd_dq_split<64, true>, attn_bwd_dkdv8<64, true>, attn_bwd_gqa_reduce<64>)
                : run(attn_bwd_dq_split<64, false>, attn_bwd_dkdv8<64, false>, attn_bwd_gqa_reduce<64>);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

extern "C" int kfamd_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int H, int T,
                                   int D, float scale, int causal, const long long* strides, void* stream) {
  return attn_fwd_launch(q, k, v, o, lse, B, H, H, T, D, scale, causal, strides, stream);
}

extern "C" long long kfamd_attn_bwd_workspace(int B, int H, int T, int D) {
  return 2LL * B * H * T * 4;  // nl, nd f32 [B][H][T]
}

// strides: 8 tensors x (b, h, t): q, k, v, o, do, dq, dk, dv. workspace: kfamd_attn_bwd_workspace bytes
// (16-B aligned): the row constants nl / nd that the dQ kernel writes for the dK / dV kernel. Written before
// it is read; its contents on entry do not matter.
extern "C" int kfamd_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                   const void* lse, void* dq, void* dk, void* dv, void* workspace, int B, int H, int T,
                                   int D, float scale, int causal, const long long* strides, void* stream) {
  return attn_bwd_launch(q, k, v, o, dout, lse, dq, dk, dv, workspace, B, H, H, T, D, scale, causal, 0, strides, stream);
}

// ---- grouped K / V heads (kfamd_kernels.h) ----
extern "C" int kfamd_attn_fwd_gqa_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int H,
                                       int Hkv, int T, int D, float scale, int causal, const long long* strides,
                                       void* stream) {
  return attn_fwd_launch(q, k, v, o, lse, B, H, Hkv, T, D, scale, causal, strides, stream);
}

extern "C" int kfamd_attn_bwd_gqa_group_split(int B, int H, int Hkv, int T, int D) {
  if (B <= 0 || H <= 0 || T <= 0 || (D != 64 && D != 128) || Hkv < 1 || H % Hkv != 0) return KFAMD_EINVAL;
  return gqa_group_split(B, H, Hkv, T, D);
}

extern "C" long long kfamd_attn_bwd_gqa_workspace(int B, int H, int Hkv, int T, int D, int group_split) {
  const int rule = kfamd_attn_bwd_gqa_group_split(B, H, Hkv, T, D);
  if (rule < 0) return KFAMD_EINVAL;
  const int G = H / Hkv;
  if (group_split < 0 || (group_split > 0 && G % group_split != 0)) return KFAMD_EINVAL;
  if (Hkv == H) return kfamd_attn_bwd_workspace(B, H, T, D);
  const int gs = group_split > 0 ? group_split : rule;
  // nl, nd f32 [B][H][T], then (GS < G) the parts' fp32 sums [dk, dv][G / GS][B][Hkv][T][D]
  return align16(2LL * B * H * T * 4) + (gs == G ? 0LL : 2LL * (G / gs) * B * Hkv * T * D * 4);
}

extern "C" int kfamd_attn_bwd_gqa_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                       const void* lse, void* dq, void* dk, void* dv, void* workspace, int B, int H,
                                       int Hkv, int T, int D, float scale, int causal, int group_split,
                                       const long long* strides, void* stream) {
  return attn_bwd_launch(q, k, v, o, dout, lse, dq, dk, dv, workspace, B, H, Hkv, T, D, scale, causal, group_split,
                         strides, stream);
}
