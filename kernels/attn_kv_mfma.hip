// attn_kv_mfma.hip — chunked-prefill attention: MFMA query tiles over the KV cache (bf16 or FP8 cache).
//
// The contract of attn_kv.hip's extend kernels without the row limit: Tq >= 1 query rows per (batch, head),
// already appended to the cache [B][H][Tcap][D], row i attends keys 0 .. lens[b] - Tq + i. lens is DEVICE
// memory and is never advanced; the grid is sized from the host's t_bound. A row whose limit is negative
// gives zeros and lse = -inf. Cache rows at or beyond lens[b] may hold NaN (bf16) or code 0x7F and NaN
// scales (FP8) and never reach the result.
//
// attn_chunk_split<Fmt, D>: one workgroup = 4 waves = one tile of kTileRows = 128 query rows of one
// (b, h) and one split of the keys. Each wave owns 32 query rows, Q in registers; the waves share K / V
// tiles of 64 keys, double-buffered in the swizzled LDS image of attention_bf16.hip's forward and staged
// through registers (loads issued before a tile's products, written after them). Per 64-key tile and wave,
// as in that forward (lane maps: its header, and cdna_hip_programming.md "An accumulator tile as the next
// MFMA's operand"):
//     S^T[key][q]  = K . Q^T        v_mfma_f32_32x32x16_bf16, A = K rows (ds_read_b128), B = Q
//     O^T[d][q]   += V^T . P^T      A = V columns (ds_read_b64_tr_b16), B = P^T: the S^T accumulator
//                                   converted to bf16 in registers (the query is on the lane, so the
//                                   online softmax of a row stays in its lane pair: v_permlane32_swap)
// A wave whose 32 rows all lie at or beyond Tq takes part in the loads and barriers and skips the math; so
// does a wave on a key tile that begins beyond its last row's limit.
//
// Masking. Only key tiles that reach past the wave's lowest limit take the per-element mask (key > limit
// -> -inf, by select); the tiles below it run unmasked. P = 0 does not protect the P.V MFMA from a NaN in V
// (0 * NaN = NaN), so nothing at or beyond lens[b] is ever staged: K, V and the FP8 scales are read by
// range-checked buffer loads over the (b, h) slice whose range ends at row lens[b] — a row past it reads
// as zero in the address unit, no memory access, no branch. (Keys between a row's limit and lens[b] are
// the block's own later rows: finite, and masked by the select.) A row that has seen no key keeps
// m = -inf; the softmax's reference is then 0 by select, so no inf - inf is formed.
//
// FP8 cache (Fp8Rows): the arithmetic rule of the VALU kernels. The codes are widened to bf16 while
// staging (exact), the fp32 score of key j is (q . codes_k[j]) * kscale[j], and vscale[j] is multiplied
// into p before the bf16 conversion. The tile's 64 + 64 scales ride through LDS next to the tile. Nothing
// dequantised is written to memory. Rounding p * vscale to bf16 moves each weight by up to 2^-8 of itself,
// and unlike the bf16 cache's p (exactly 1 for a row that sees one key) the product is never exact: divided
// by the sum l of the unrounded p, a row dominated by one key came out off by up to 2^-8 |v|. So next to l
// (which the lse and the split records need) the kernel sums lw, the weights P.V really used —
// bf16(p * vscale) / vscale, the reciprocal staged with the scales — and scales O by l / lw at the end: the
// row is then sum(w v) / sum(w) with the rounded weights, a convex combination, exact for a one-key row.
//
// Split over keys, from host-known values only (a captured step replays): tiles = ceil(Tq / 128),
// nsplit = clamp(ceil(256 / (tiles * H * B)), 1, ceil(t_bound / kSplitKeys)) — 256 is the chip's CU count —
// and every split covers ceil(ceil(t_bound / kSplitKeys) / nsplit) * kSplitKeys keys. With one split the
// kernel writes the bf16 rows and the lse; otherwise it writes attn_kv.hip's (m, l, o[D]) fp32 records
// and attn_kv_combine<D> merges them (gridDim.z = Tq, hence Tq <= 65535): two dependent launches, no
// atomics, no cross-workgroup waiting, results bitwise repeatable. The workspace is B * H * Tq * nsplit *
// (D + 2) * 4 bytes; more than one split means tiles * H * B < 256, so rows * nsplit stays below
// 2 * 256 * 128 and the workspace below 2 * 256 * 128 * (D + 2) * 4 bytes: 34.1 MB at D = 128, 17.3 MB
// at D = 64.
//
// Grouped-query attention (attn_chunk_split<Fmt, D, true>, the kfamd_attn_chunk_gqa_* entry points): the grid's
// h is a K / V head and the kernel tiles its T * G rows, flattened token-major (r = t * G + g, limit
// lens[b] - T + r / G). 32 and 128 are multiples of every G in {1, 2, 4, 8, 16}, so a token's heads never
// straddle a wave or a tile, and the limit is non-decreasing in r, so the tile's last row and the wave's
// first row still give the highest and the lowest limit. The split count is the rule above with
// tiles = ceil(T * G / 128) and H := Hkv, T * G <= 65535, the workspace B * Hkv * (T * G) * nsplit * (D + 2) * 4
// bytes. The GQ = false instantiations are the kernels as they were; G = 1 launches them.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 for all:
//   instantiation                               VGPRs   LDS bytes
//   attn_chunk_split<Bf16Rows, 64, false>        124   32768
//   attn_chunk_split<Bf16Rows, 128, false>       232   65536
//   attn_chunk_split<Fp8Rows, 64, false>         184   34304
//   attn_chunk_split<Fp8Rows, 128, false>        254   67072
//   attn_chunk_split<Bf16Rows, 64, true>         126   32768
//   attn_chunk_split<Bf16Rows, 128, true>        234   65536
//   attn_chunk_split<Fp8Rows, 64, true>          185   34304
//   attn_chunk_split<Fp8Rows, 128, true>         255   67072
// WIN = true (sliding window, kfamd_attn_chunk_win_*; the comment at the kernel): 125 / 233 / 184 / 254 VGPRs for
// <Bf16Rows, 64>, <Bf16Rows, 128>, <Fp8Rows, 64>, <Fp8Rows, 128> plain and 126 / 234 / 185 / 255 grouped, the same LDS,
// scratch 0. The zero-staging of the rows below the window is in the first tile's stage_write only: in every
// tile's it spilled <Fp8Rows, 128> (256 VGPRs, 8 - 12 B scratch).
// RING = true (ring-buffer cache, kfamd_attn_chunk_ring_*; the comment at the kernel), scratch 0 for all:
//   attn_chunk_split<Bf16Rows, 64, false, true, true>      125   32768
//   attn_chunk_split<Bf16Rows, 128, false, true, true>     233   65536
//   attn_chunk_split<Fp8Rows, 64, false, true, true>       184   34304
//   attn_chunk_split<Fp8Rows, 128, false, true, true>      254   67072
//   attn_chunk_split<Bf16Rows, 64, true, true, true>       126   32768
//   attn_chunk_split<Bf16Rows, 128, true, true, true>      234   65536
//   attn_chunk_split<Fp8Rows, 64, true, true, true>        185   34304
//   attn_chunk_split<Fp8Rows, 128, true, true, true>       255   67072
// PAGED = true (a paged cache, kfamd_attn_chunk_paged_*; the comment at the kernel), scratch 0 for all:
//   attn_chunk_split<Bf16Rows, 64, false, false, false, true>     125   32768
//   attn_chunk_split<Bf16Rows, 128, false, false, false, true>    233   65536
//   attn_chunk_split<Fp8Rows, 64, false, false, false, true>      185   34304
//   attn_chunk_split<Fp8Rows, 128, false, false, false, true>     255   67072
//   attn_chunk_split<Bf16Rows, 64, true, false, false, true>      127   32768
//   attn_chunk_split<Bf16Rows, 128, true, false, false, true>     235   65536
//   attn_chunk_split<Fp8Rows, 64, true, false, false, true>       186   34304
//   attn_chunk_split<Fp8Rows, 128, true, false, false, true>      256   67072
// The grouped limit is no affine function of the row, and with both kept through the key loop
// <Fp8Rows, 128, true> spilled (256 VGPRs, 8 B scratch): the masked tiles compute the limit again instead.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "attn_kv_rows.h"
#include "attn_tile.h"
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

using namespace kfa;
using kfkv::kLn2;
using kfkv::kLog2e;
using kfkv::kSplitKeys;

constexpr int kTileRows = 128;  // query rows per workgroup: 4 waves x 32
constexpr int kThreads = 256;
constexpr int FK = 64;          // keys per K / V tile
constexpr int kCUs = 256;       // compute units of the chip: what the split count fills
constexpr int kMaxRows = 65535;  // attn_kv_combine takes the row in gridDim.z

struct ChunkArgs {
  const __bf16* q;
  const void* k;  // Fmt::Elem
  const void* v;
  const float* ks;  // Fmt::kScaled only, as ksb .. vsh
  const float* vs;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int B, H, Tq, t_bound, nsplit, split_keys;  // split_keys: keys per split, a multiple of kSplitKeys
  float scale_log2;
  int lg;  // GQ kernels only: log2 of the group size G. H is then Hkv and Tq the T * G flattened rows
  long long qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh, ksb, ksh, vsb, vsh;
  int window;  // WIN kernels only: the sliding window W >= 1
  int cap;     // RING kernels only: the ring's capacity C, a multiple of kSplitKeys
};

// PAGED kernels (the page rule: the docstring of ops/decode.py): the flat arguments, with the page stride of K, V and
// the scales in kb, vb, ksb, vsb, plus the page table. A type of its own, so that the flat kernels' argument block (and
// with it their code) stays as it was.
struct PagedChunkArgs : ChunkArgs {
  const int* pt;  // device int32 [B][pts]: the page of keys 256 c .. 256 c + 255 of row b, -1 for none
  long long pts;
  int n_pages;
};

template <class Vec>
__device__ __forceinline__ Vec bload8(__amdgpu_buffer_rsrc_t r, int byte_off, int soff) {
  if constexpr (sizeof(Vec) == 16) return bload16(r, byte_off, soff);
  else return __builtin_bit_cast(Vec, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, soff, 0));
}

// workspace: attn_kv.hip's, [B][H][Tq][nsplit][2] (m, l) then [B][H][Tq][nsplit][D] (o), fp32
// GQ (grouped-query attention): h is a K / V head and the Tq rows are its T * G (token, head-in-group) pairs
// flattened token-major, r = t * G + g with G = 1 << lg: token r >> lg of query head (h << lg) + (r & (G - 1)),
// limit len - T + (r >> lg). The limit is non-decreasing in r, so the tile's last row still has the tile's
// highest limit and a wave's first row its lowest; 32 and 128 are multiples of G.
// WIN (sliding window, the rule: ops/decode.py): a row of limit lim sees keys max(0, lim + 1 - W) .. lim. The lower
// bound is non-decreasing in r like the limit: the tile's first row has the tile's lowest, a wave's first and last
// real rows its lowest and highest. The key loop starts at the tile of 64 keys that holds the tile's lowest lower
// bound blo; keys below blo may be poison and are staged as zeros (P = 0 would not keep a NaN of V out of P.V),
// keys from blo on are some row's and finite, masked per element by select on the tiles that cross a row's bound.
// RING (a ring-buffer cache, the rule: ops/decode.py): key j lives in slot j % C, lens is absolute, and the split
// partition is rebased at base_b, the 256-aligned split that holds the call's lowest lower bound. C is a multiple of
// 256, so a 64-key tile is one run of slots: the tile's scalar row offset advances by 64 with a conditional subtract
// of C. The slice is all C rows, and the slots after key len - 1 hold the oldest live keys, or stale or poisoned rows:
// the rows of the LAST tile at or beyond len (only the last tile can hold them) must reach LDS as zeros, for K, V and
// the FP8 scales. That tile is one run of slots that ends inside the slice, so its loads go through descriptors whose
// range ends at its row len - key0: the address unit returns zeros beyond it, as it does past row len of a flat cache,
// at the cost of scalar registers only. (A select in stage_write, as for the first tile's rows below blo, spilled
// <Fp8Rows, 128>: 256 VGPRs, 24 - 32 B scratch.)
// PAGED (a paged cache, the rule: ops/decode.py): key j lives in page pt[b][j >> 8] at row j & 255. A split spans
// several pages, a 64-key tile lies in one: stage_load reads the tile's page id as a block-uniform scalar (clamped into
// [0, n_pages - 1]; only tiles that begin below len are staged, so an absent entry is never read) and rebuilds the K, V
// and scale descriptors on that page's (page, h) slice. Their range ends at row min(256, len - page's first key): the
// rows at or beyond len read as zeros from the address unit, as on the flat cache and the ring's last tile.
template <class Fmt, int D, bool GQ, bool WIN, bool RING, bool PAGED>
__global__ __launch_bounds__(kThreads, 2) void attn_chunk_split(std::conditional_t<PAGED, PagedChunkArgs, ChunkArgs> a) {
  static_assert(WIN || !RING, "a ring always has a window");
  static_assert(!PAGED || !WIN, "a paged cache has neither a window nor a ring");
  typedef typename Fmt::Elem Elem;
  typedef typename Fmt::Vec Vec;
  constexpr int KS = D / 16;               // k-steps of the Q K^T product
  constexpr int ND = D / 32;               // 32-wide d tiles of O
  constexpr int CH = D / 8;                // 8-element chunks per row
  constexpr int NCH = FK * CH / kThreads;  // chunks per thread per K (and per V) tile
  constexpr int TILE = FK * D * 2;         // bytes of one K (or V) tile image
  constexpr int ES = (int)sizeof(Elem);
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];                   // [buf][K, V]
  __shared__ __attribute__((aligned(16))) float s_sc[Fmt::kScaled ? 2 : 1][3][FK];  // [buf][k, v, 1 / v][key]

  const int tile = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = a.Tq, nsplit = a.nsplit;
  const int lg = GQ ? a.lg : 0, gmask = (1 << lg) - 1;
  const int T = Tq >> lg, Hq = a.H << lg, h0 = h << lg;  // tokens, query heads, the group's first query head

  int len = a.lens[b];
  if constexpr (RING) len = max(len, 0);  // absolute, not bounded by the capacity
  else len = len < 0 ? 0 : (len > a.t_bound ? a.t_bound : len);
  const int q0 = tile * kTileRows, qw = q0 + 32 * w, qrow = qw + r;
  const int qlast = min(q0 + kTileRows, Tq) - 1;  // the tile's last row
  int k0 = split * a.split_keys;
  if constexpr (RING) k0 += max(len - T + 1 - a.window, 0) / kSplitKeys * kSplitKeys;  // + base_b
  const int k1 = min(k0 + a.split_keys, len - T + (qlast >> lg) + 1);  // keys of this split that the last row sees: [k0, k1)
  const long long bh = (long long)b * a.H + h;
  const long long nrows = (long long)a.B * a.H * Tq;
  float* ws_o = a.ws + nrows * nsplit * 2;
  int blo = 0;  // WIN: the lowest lower bound of the tile's rows, its first row's
  if constexpr (WIN) blo = max(len - T + (q0 >> lg) + 1 - a.window, 0);

  if (k1 <= k0 || (WIN && blo >= k1)) {  // no key for any row of the tile (block-uniform, before any barrier)
    for (int item = tid; item < (qlast - q0 + 1) * D; item += kThreads) {
      const int rr = q0 + item / D, d = item % D;
      const long long row = bh * Tq + rr;
      if (nsplit > 1) {
        ws_o[(row * nsplit + split) * D + d] = 0.f;
        if (d == 0) *reinterpret_cast<float2*>(a.ws + (row * nsplit + split) * 2) = make_float2(-INFINITY, 0.f);
      } else {
        a.o[b * a.ob + (rr >> lg) * a.ot + (h0 + (rr & gmask)) * a.oh + d] = (__bf16)0.f;
        if (d == 0 && a.lse) a.lse[((long long)b * T + (rr >> lg)) * Hq + h0 + (rr & gmask)] = -INFINITY;
      }
    }
    return;
  }

  // this lane's row sees keys 0 .. lim; a padding row (>= Tq) and a row before the sequence's start see none
  // GQ: the limit is no affine function of the row, and Fp8Rows at D = 128 has no VGPR to keep both through
  // the key loop: the masked tiles (few: those that reach past the wave's lowest limit) compute it again
  const int lim = qrow < Tq ? len - T + (qrow >> lg) : -1;
  const bool wave_live = qw < Tq;                                   // wave-uniform: the wave holds a real row
  const int wave_lo = qw + 31 < Tq ? len - T + (qw >> lg) : -1;     // the wave's lowest limit
  const int wave_hi = len - T + (min(qw + 31, Tq - 1) >> lg);       // and its highest
  int wave_blo = 0, wave_bhi = 0;  // WIN: the lowest and the highest lower bound of the wave's real rows
  if constexpr (WIN) {
    wave_blo = max(len - T + (qw >> lg) + 1 - a.window, 0);
    wave_bhi = max(wave_hi + 1 - a.window, 0);
  }

  bf16x8 qf[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    u32x4 x = {0u, 0u, 0u, 0u};
    if (qrow < Tq) x = gload16(a.q + b * a.qb + (qrow >> lg) * a.qt + (h0 + (qrow & gmask)) * a.qh + kk * 16 + 8 * hh);
    qf[kk] = __builtin_bit_cast(bf16x8, x);
  }

  // the (b, h) slices end at row len: whatever lies at or beyond it reads as zero
  const Elem* kbase = static_cast<const Elem*>(a.k) + (PAGED ? 0 : b * a.kb) + h * a.kh;  // PAGED: + page * kb per tile
  const Elem* vbase = static_cast<const Elem*>(a.v) + (PAGED ? 0 : b * a.vb) + h * a.vh;
  const int kt = (int)a.kt, vt = (int)a.vt;
  const auto rk0 = slice_rsrc(kbase, (long long)len * kt * ES), rv0 = slice_rsrc(vbase, (long long)len * vt * ES);
  const auto rs0 = slice_rsrc(Fmt::kScaled ? (w == 0 ? a.ks + b * a.ksb + h * a.ksh : a.vs + b * a.vsb + h * a.vsh)
                                          : nullptr,
                             Fmt::kScaled ? 4LL * len : 0);
  int slot = 0;  // RING: the slot of the next tile staged (block-uniform); tiles are staged in order
  Vec kreg[NCH], vreg[NCH];
  float screg = 0.f;  // Fmt::kScaled: wave 0 carries the tile's 64 K scales, wave 1 its V scales
  auto stage_load = [&](int key0) {
    auto rk = rk0, rv = rv0, rs = rs0;  // the flat cache's descriptors: their range ends at row len
    if constexpr (RING) {  // the tile's offsets come from the slot, never from the absolute key index
      // the slice's rows in range: all C, but for the last tile those below slot + (len - key0)
      const int rows = key0 + FK > len ? slot + len - key0 : a.cap;
      rk = slice_rsrc(kbase, (long long)rows * kt * ES), rv = slice_rsrc(vbase, (long long)rows * vt * ES);
      if constexpr (Fmt::kScaled)
        rs = slice_rsrc(w == 0 ? a.ks + b * a.ksb + h * a.ksh : a.vs + b * a.vsb + h * a.vsh, 4LL * rows);
      key0 = slot;
      slot += FK;
      if (slot >= a.cap) slot -= a.cap;
    }
    if constexpr (PAGED) {  // the tile's page: its slice, in range up to the row that holds key len - 1
      const long long page = min(max(a.pt[b * a.pts + (key0 >> 8)], 0), a.n_pages - 1);
      const int rows = min(kSplitKeys, len - (key0 & ~(kSplitKeys - 1)));
      rk = slice_rsrc(kbase + page * a.kb, (long long)rows * kt * ES);
      rv = slice_rsrc(vbase + page * a.vb, (long long)rows * vt * ES);
      if constexpr (Fmt::kScaled)
        rs = slice_rsrc(w == 0 ? a.ks + page * a.ksb + h * a.ksh : a.vs + page * a.vsb + h * a.vsh, 4LL * rows);
      key0 &= kSplitKeys - 1;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + kThreads * i, row = c / CH, ch = c % CH;
      // the lane's part in the voffset, the tile's row offset in the (scalar) soffset
      kreg[i] = bload8<Vec>(rk, ES * (row * kt + ch * 8), ES * key0 * kt);
      vreg[i] = bload8<Vec>(rv, ES * (row * vt + ch * 8), ES * key0 * vt);
    }
    if constexpr (Fmt::kScaled) {
      if (w < 2) screg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, 4 * lane, 4 * key0, 0));
    }
  };
  // cut (WIN, the first tile only: every later one begins beyond blo): the tile's rows below it lie below every
  // row's window and are staged as zeros; 0 for every other tile, a constant the selects fold away on
  auto stage_write = [&](int buf, int cut) __attribute__((always_inline)) {
    char* kimg = smem + buf * 2 * TILE;
    char* vimg = kimg + TILE;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + kThreads * i, row = c / CH, ch = c % CH;
      const int off = img_off<D>(row, ch);
      if constexpr (WIN) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(kimg + off) = row < cut ? zero : Fmt::to_bf16(kreg[i]);
        *reinterpret_cast<u32x4*>(vimg + off) = row < cut ? zero : Fmt::to_bf16(vreg[i]);
      } else {  // the statements as they were: the same instruction order as before the window
        *reinterpret_cast<u32x4*>(kimg + off) = Fmt::to_bf16(kreg[i]);
        *reinterpret_cast<u32x4*>(vimg + off) = Fmt::to_bf16(vreg[i]);
      }
    }
    if constexpr (Fmt::kScaled) {
      if constexpr (WIN) {
        if (lane < cut) screg = 0.f;  // as a row past the slice
      }
      if (w < 2) s_sc[buf][w][lane] = screg;
      if (w == 1) s_sc[buf][2][lane] = screg != 0.f ? 1.f / screg : 0.f;  // 0: a row past the slice
    }
  };

  const float c = a.scale_log2;
  float m = -INFINITY, l = 0.f;  // m in log2 units of the scaled score, as the split records hold it
  float lw = 0.f;                // Fmt::kScaled: the sum of the weights P.V really used (see the header)
  f32x16 oacc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) oacc[n] = (f32x16){};

  // k0 is a multiple of kSplitKeys, so of FK. WIN: the first tile is the one that holds blo
  const int j0 = (WIN ? max(k0, blo) : k0) / FK, j1 = (k1 + FK - 1) / FK;
  if constexpr (RING) slot = j0 * FK % a.cap;
  stage_load(j0 * FK);
  stage_write(0, WIN ? blo - j0 * FK : 0);
  __syncthreads();

  // per-lane LDS offsets of every operand read, computed once; what varies per read is compile-time
  int koff[KS], voff0[ND], voff1[ND];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) koff[kk] = img_off<D>(r, 2 * kk + hh);  // + 32 t rows: swizzle bits unchanged
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3;
    const int r0 = 4 * hh + qq;  // + a multiple of 16 rows: swizzle bits unchanged
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int col = 32 * n + 16 * (g & 1) + 4 * pp;
      voff0[n] = img_off<D>(r0, col >> 3) + 8 * (pp & 1);
      voff1[n] = img_off<D>(r0 + 8, col >> 3) + 8 * (pp & 1);
    }
  }

  auto tile_body = [&](int j, auto BUFC) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUFC)::value;
    const int key0 = j * FK;
    const bool more = j + 1 < j1;
    if (more) stage_load(key0 + FK);
    const char* kimg = smem + BUF * 2 * TILE;
    const char* vimg = kimg + TILE;
    if (wave_live && key0 <= wave_hi && (!WIN || key0 + FK - 1 >= wave_blo)) {  // wave-uniform
      f32x16 sacc[2] = {(f32x16){}, (f32x16){}};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
        for (int t = 0; t < 2; ++t) sacc[t] = mfma32(lds_row(kimg + 32 * t * D * 2, koff[kk]), qf[kk], sacc[t]);
      }
      // element e of sacc[t] is key key0 + 32 t + (e & 3) + 8 (e >> 2) + 4 hh: runs of 4 keys per register quad
      if constexpr (Fmt::kScaled) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(&s_sc[BUF][0][32 * t + 8 * g + 4 * hh]);
#pragma unroll
            for (int x = 0; x < 4; ++x) sacc[t][4 * g + x] *= s4[x] * c;
          }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) sacc[t] *= c;
      }
      // the tile reaches past some row's limit (WIN: or begins below some row's lower bound)
      if (key0 + FK - 1 > wave_lo || (WIN && key0 < wave_bhi)) {
        int mlim = lim;
        if constexpr (GQ) {
          int qr = qrow;
          asm volatile("" : "+v"(qr));  // not hoisted out of the key loop
          mlim = qr < Tq ? len - T + (qr >> lg) : -1;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = key0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
            if constexpr (WIN) sacc[t][e] = key > mlim || key < mlim + 1 - a.window ? -INFINITY : sacc[t][e];
            else sacc[t][e] = key > mlim ? -INFINITY : sacc[t][e];
          }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sacc[t][e]);
      mx = kfw::max_halves(mx);  // the row's other 32 keys
      const float mn = fmaxf(m, mx);
      const float mref = mn == -INFINITY ? 0.f : mn;  // a row with no key so far: every p below is exp2(-inf) = 0
      // O and l are rescaled only when some row's max grew (exact: alpha == 1 otherwise)
      const bool grew = __builtin_amdgcn_ballot_w64(mx > m) != 0;
      const float alpha = grew ? fast_exp2(m - mref) : 1.f;
      m = mn;
      float rsum = 0.f, wsum = 0.f;
      uint32_t pf[2][2][4];  // [t][s][pair]: P^T as the B operand of P.V
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 v4[4], iv4[4];
        if constexpr (Fmt::kScaled) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            v4[g] = *reinterpret_cast<const f32x4*>(&s_sc[BUF][1][32 * t + 8 * g + 4 * hh]);
            iv4[g] = *reinterpret_cast<const f32x4*>(&s_sc[BUF][2][32 * t + 8 * g + 4 * hh]);
          }
        }
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          float p0 = fast_exp2(sacc[t][e] - mref);
          float p1 = fast_exp2(sacc[t][e + 1] - mref);
          rsum += p0 + p1;
          if constexpr (Fmt::kScaled) {  // V's scale folded into p
            p0 *= v4[e >> 2][e & 3];
            p1 *= v4[e >> 2][(e & 3) + 1];
          }
          const uint32_t pw2 = pack2(p0, p1);
          pf[t][e >> 3][(e & 7) >> 1] = pw2;
          if constexpr (Fmt::kScaled) {  // the rounded p * vscale, taken back to a probability
            wsum = fmaf(__uint_as_float(pw2 << 16), iv4[e >> 2][e & 3], wsum);
            wsum = fmaf(__uint_as_float(pw2 & 0xffff0000u), iv4[e >> 2][(e & 3) + 1], wsum);
          }
        }
      }
      if constexpr (Fmt::kScaled) lw = grew ? lw * alpha + wsum : lw + wsum;
      if (grew) {
        l = l * alpha + rsum;
#pragma unroll
        for (int n = 0; n < ND; ++n) oacc[n] *= alpha;
      } else {
        l += rsum;
      }
#pragma unroll
      for (int n = 0; n < ND; ++n) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const char* vrows = vimg + (32 * t + 16 * s) * D * 2;
            const bf16x8 vf = join(tr_read(vrows, voff0[n]), tr_read(vrows, voff1[n]));
            const u32x4 pw = {pf[t][s][0], pf[t][s][1], pf[t][s][2], pf[t][s][3]};
            oacc[n] = mfma32(vf, __builtin_bit_cast(bf16x8, pw), oacc[n]);
          }
        }
      }
    }
    if (more) stage_write(1 - BUF, 0);
    __syncthreads();
  };
  for (int j = j0; j < j1; j += 2) {
    tile_body(j, std::integral_constant<int, 0>{});
    if (j + 1 < j1) tile_body(j + 1, std::integral_constant<int, 1>{});
  }

  // epilogue: lane (r, hh) holds row qrow, d = 32 n + (e & 3) + 8 (e >> 2) + 4 hh; both halves hold m
  if (!wave_live) return;
  const float lt = kfw::sum_halves(l);
  if constexpr (Fmt::kScaled) {  // O / lw is the row; what follows divides by l
    const float lwt = kfw::sum_halves(lw);
    const float adj = lwt > 0.f ? lt / lwt : 1.f;
#pragma unroll
    for (int n = 0; n < ND; ++n) oacc[n] *= adj;
  }
  if (qrow >= Tq) return;
  const int qtok = qrow >> lg, qhead = h0 + (qrow & gmask);  // where the row lives in o and lse
  const long long row = bh * Tq + qrow;
  if (nsplit > 1) {  // m = -inf, l = 0, o = 0 for a row with no key in this split
    float* po = ws_o + (row * nsplit + split) * D;
#pragma unroll
    for (int n = 0; n < ND; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float* p = po + 32 * n + 8 * g + 4 * hh;  // 8-B aligned: the records begin 8 * nrows * nsplit bytes in
        *reinterpret_cast<float2*>(p) = make_float2(oacc[n][4 * g], oacc[n][4 * g + 1]);
        *reinterpret_cast<float2*>(p + 2) = make_float2(oacc[n][4 * g + 2], oacc[n][4 * g + 3]);
      }
    if (hh == 0) *reinterpret_cast<float2*>(a.ws + (row * nsplit + split) * 2) = make_float2(m, lt);
  } else {
    const bool any = lt > 0.f;  // a row before the sequence's start (lens[b] < Tq) sees no key
    const float inv = any ? 1.f / lt : 0.f;
    __bf16* ob = a.o + b * a.ob + qtok * a.ot + qhead * a.oh;
#pragma unroll
    for (int n = 0; n < ND; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x2 v2 = {pack2(oacc[n][4 * g] * inv, oacc[n][4 * g + 1] * inv),
                          pack2(oacc[n][4 * g + 2] * inv, oacc[n][4 * g + 3] * inv)};
        *reinterpret_cast<u32x2*>(ob + 32 * n + 8 * g + 4 * hh) = v2;
      }
    if (hh == 0 && a.lse) a.lse[((long long)b * T + qtok) * Hq + qhead] = any ? (m + log2f(lt)) * kLn2 : -INFINITY;
  }
}

int chunk_tiles(int Tq) { return (Tq + kTileRows - 1) / kTileRows; }

// the split count: fills the chip's compute units, from host-known values only
int chunk_nsplit(int B, int H, int Tq, int t_bound) {
  const long long wgs = (long long)chunk_tiles(Tq) * H * B;
  const long long want = wgs >= kCUs ? 1 : (kCUs + wgs - 1) / wgs;
  const long long most = (t_bound + kSplitKeys - 1) / kSplitKeys;
  return (int)(want < most ? want : most);
}

bool chunk_shape_ok(int B, int H, int D, int Tq, int t_bound) {
  return B > 0 && H > 0 && B <= 65535 && H <= 65535 && (D == 64 || D == 128) && Tq >= 1 && Tq <= kMaxRows &&
         t_bound >= 1;
}

// the grouped forms: Hkv K / V heads, G in {1, 2, 4, 8, 16} query heads on each, T tokens, T * G <= 65535 rows
bool chunk_gqa_ok(int B, int Hkv, int G, int D, int T, int t_bound) {
  const int lg = kfkv::group_log2(G);
  return lg >= 0 && T >= 1 && T <= (kMaxRows >> lg) && chunk_shape_ok(B, Hkv, D, T << lg, t_bound);
}

template <class Fmt, bool WIN, bool RING, bool PAGED = false, class Args = ChunkArgs>
void launch_chunk(const Args& a, int D, dim3 grid, hipStream_t s) {
  const dim3 block(kThreads);
  if (a.lg > 0 && D == 64)
    hipLaunchKernelGGL((attn_chunk_split<Fmt, 64, true, WIN, RING, PAGED>), grid, block, 0, s, a);
  else if (a.lg > 0) hipLaunchKernelGGL((attn_chunk_split<Fmt, 128, true, WIN, RING, PAGED>), grid, block, 0, s, a);
  else if (D == 64) hipLaunchKernelGGL((attn_chunk_split<Fmt, 64, false, WIN, RING, PAGED>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((attn_chunk_split<Fmt, 128, false, WIN, RING, PAGED>), grid, block, 0, s, a);
}

// keys a ring launch partitions: the ceil((W + T - 1) / 256) + 1 splits of 256 from base_b on (attn_kv.hip's count)
int ring_span(int window, int T) {
  return (int)((((long long)window + T - 1 + kSplitKeys - 1) / kSplitKeys + 1) * kSplitKeys);
}

// The launcher behind kfamd_attn_chunk_bf16 / _fp8. window: 0 for the entry points without one, else W >= 1. st: q (b, t, h), k (b, h, t), v (b, h, t), o (b, t, h),
// then for a scaled format k_scale (b, h), v_scale (b, h). Every KFAMD_EINVAL condition is tested before
// any KFAMD_EALIGN one. The grouped entry points pass G > 0: H is then Hkv, Tq the token count T, the q / o
// strides' h runs over the Hkv * G query heads and the kernel tiles the T * G rows of a K / V head (the split
// count and the workspace follow from Hkv and T * G); G = 1 there launches what the plain entry points launch.
template <class Fmt>
int attn_chunk(const void* q, const void* k, const void* v, const float* ks, const float* vs, const int* lens,
               void* o, float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
               const long long* st, void* stream, int G = 0, int window = 0, bool ring = false,
               const int* pt = nullptr, long long pts = 0, int n_pages = 0) {
  // paged (pt given): the b strides are page strides, the table holds a column for every 256 keys of t_bound
  if (pt && (n_pages < 1 || window > 0 || ring || t_bound < 1 || pts < (t_bound + kSplitKeys - 1) / kSplitKeys ||
             !kfkv::al4(pt)))
    return KFAMD_EINVAL;
  // ring: t_bound is the capacity C (the limit checks below then bound the slice of C rows), and the split count and
  // the keys per split come from the span of W and T, never from a position
  if (ring && (window < 1 || t_bound < 1 || t_bound % kSplitKeys || Tq < 1 || (long long)window + Tq - 1 > t_bound))
    return KFAMD_EINVAL;
  const int span = ring ? ring_span(window, Tq) : t_bound;
  if (window < 0 || (G > 0 && !chunk_gqa_ok(B, H, G, D, Tq, t_bound))) return KFAMD_EINVAL;
  const int lg = G > 0 ? kfkv::group_log2(G) : 0;
  Tq <<= lg;  // rows per (b, K / V head) from here on
  if (!q || !k || !v || !lens || !o || !st || !chunk_shape_ok(B, H, D, Tq, t_bound)) return KFAMD_EINVAL;
  if (Fmt::kScaled && (!ks || !vs)) return KFAMD_EINVAL;
  ChunkArgs a = {};
  a.qb = *st++, a.qt = *st++, a.qh = *st++;
  a.kb = *st++, a.kh = *st++, a.kt = *st++, a.vb = *st++, a.vh = *st++, a.vt = *st++;
  a.ob = *st++, a.ot = *st++, a.oh = *st++;
  if (Fmt::kScaled) a.ksb = *st++, a.ksh = *st++, a.vsb = *st++, a.vsh = *st++;
  if (a.kt < D || a.vt < D) return KFAMD_EINVAL;
  const long long lim = (1ll << 31) / (long long)sizeof(typename Fmt::Elem);  // a (b, h) slice stays below 2^31 bytes
  if ((long long)t_bound * a.kt >= lim || (long long)t_bound * a.vt >= lim) return KFAMD_EINVAL;
  a.nsplit = chunk_nsplit(B, H, Tq, span);
  const long long wgs = (long long)chunk_tiles(Tq) * a.nsplit;
  if (wgs > 0x7fffffffll || (a.nsplit > 1 && !ws)) return KFAMD_EINVAL;
  if (!kfkv::al16(q) || !kfkv::al16(k) || !kfkv::al16(v) || !kfkv::al16(o) || (ws && !kfkv::al16(ws)))
    return KFAMD_EALIGN;
  if (Fmt::kScaled && (!kfkv::al4(ks) || !kfkv::al4(vs))) return KFAMD_EALIGN;
  if ((a.qb | a.qt | a.qh | a.ob | a.ot | a.oh) & 7) return KFAMD_EALIGN;
  if ((a.kb | a.kh | a.kt | a.vb | a.vh | a.vt) & (Fmt::kStrideAlign - 1)) return KFAMD_EALIGN;
  a.q = static_cast<const __bf16*>(q);
  a.k = k, a.v = v, a.ks = ks, a.vs = vs, a.lens = lens;
  a.o = static_cast<__bf16*>(o);
  a.lse = lse;
  a.ws = static_cast<float*>(ws);
  a.B = B, a.H = H, a.Tq = Tq, a.t_bound = t_bound, a.lg = lg;
  a.window = ring ? window : window >= t_bound ? 0 : window;  // W >= t_bound removes no key: the kernels without a window
  a.cap = ring ? t_bound : 0;
  const int chunks = (span + kSplitKeys - 1) / kSplitKeys;
  a.split_keys = (chunks + a.nsplit - 1) / a.nsplit * kSplitKeys;
  a.scale_log2 = scale * kLog2e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)wgs, (unsigned)H, (unsigned)B);
  if (pt) {
    PagedChunkArgs pa = {};
    static_cast<ChunkArgs&>(pa) = a;
    pa.pt = pt, pa.pts = pts, pa.n_pages = n_pages;
    launch_chunk<Fmt, false, false, true>(pa, D, grid, s);
  } else if (ring) launch_chunk<Fmt, true, true>(a, D, grid, s);
  else if (a.window > 0) launch_chunk<Fmt, true, false>(a, D, grid, s);
  else launch_chunk<Fmt, false, false>(a, D, grid, s);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && a.nsplit > 1)
    e = kfkv::launch_kv_combine(D, a.ws, a.o, lse, B, H, Tq, a.nsplit, a.ob, a.ot, a.oh, s, lg);
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

}  // namespace

extern "C" int kfamd_attn_chunk_tile_rows(void) { return kTileRows; }

extern "C" int kfamd_attn_chunk_nsplit(int B, int H, int Tq, int t_bound) {
  return chunk_shape_ok(B, H, 64, Tq, t_bound) ? chunk_nsplit(B, H, Tq, t_bound) : 0;
}

extern "C" long long kfamd_attn_chunk_workspace(int B, int H, int D, int Tq, int t_bound) {
  if (!chunk_shape_ok(B, H, D, Tq, t_bound)) return 0;
  const long long nsplit = chunk_nsplit(B, H, Tq, t_bound);
  if (nsplit == 1) return 16;  // unused with one split; never 0 for an accepted shape
  return (long long)B * H * Tq * nsplit * (D + 2) * (long long)sizeof(float);
}

extern "C" int kfamd_attn_chunk_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                     float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
                                     const long long* st, void* stream) {
  return attn_chunk<kfkv::Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, H, D, Tq, t_bound,
                                    scale, st, stream);
}

extern "C" int kfamd_attn_chunk_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                    const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                    int D, int Tq, int t_bound, float scale, const long long* st, void* stream) {
  return attn_chunk<kfkv::Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, H, D, Tq, t_bound,
                                   scale, st, stream);
}

// The grouped-query forms (contract: kfamd_kernels.h).
extern "C" int kfamd_attn_chunk_gqa_nsplit(int B, int Hkv, int G, int T, int t_bound) {
  return chunk_gqa_ok(B, Hkv, G, 64, T, t_bound) ? chunk_nsplit(B, Hkv, T * G, t_bound) : 0;
}

extern "C" long long kfamd_attn_chunk_gqa_workspace(int B, int Hkv, int G, int D, int T, int t_bound) {
  return chunk_gqa_ok(B, Hkv, G, D, T, t_bound) ? kfamd_attn_chunk_workspace(B, Hkv, D, T * G, t_bound) : 0;
}

extern "C" int kfamd_attn_chunk_gqa_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                         void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                         int t_bound, float scale, const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                    scale, st, stream, G);
}

extern "C" int kfamd_attn_chunk_gqa_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                        const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                        int Hkv, int G, int D, int T, int t_bound, float scale, const long long* st,
                                        void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                   scale, st, stream, G);
}

// The sliding-window forms (contract: kfamd_kernels.h): the grouped signature, G = 1 for plain rows.
extern "C" int kfamd_attn_chunk_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                         void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                         int t_bound, int window, float scale, const long long* st, void* stream) {
  if (G <= 0 || window < 1) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                    scale, st, stream, G, window);
}

extern "C" int kfamd_attn_chunk_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                        const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                        int Hkv, int G, int D, int T, int t_bound, int window, float scale,
                                        const long long* st, void* stream) {
  if (G <= 0 || window < 1) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                   scale, st, stream, G, window);
}

// The ring forms (contract: kfamd_kernels.h): the windowed signatures with the ring's capacity C in t_bound's place.
extern "C" int kfamd_attn_chunk_ring_nsplit(int B, int Hkv, int G, int T, int window) {
  if (window < 1 || T < 1) return 0;
  return kfamd_attn_chunk_gqa_nsplit(B, Hkv, G, T, ring_span(window, T));
}

extern "C" long long kfamd_attn_chunk_ring_workspace(int B, int Hkv, int G, int D, int T, int window) {
  if (window < 1 || T < 1) return 0;
  return kfamd_attn_chunk_gqa_workspace(B, Hkv, G, D, T, ring_span(window, T));
}

extern "C" int kfamd_attn_chunk_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                          void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T, int cap,
                                          int window, float scale, const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, cap, scale,
                                    st, stream, G, window, true);
}

extern "C" int kfamd_attn_chunk_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                         const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                         int Hkv, int G, int D, int T, int cap, int window, float scale,
                                         const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, cap, scale,
                                   st, stream, G, window, true);
}

// The paged forms (contract: kfamd_kernels.h): the grouped signatures with the page table before the stream; the b
// entries of the stride array are the page strides. Split count and workspace: kfamd_attn_chunk_gqa_nsplit / _workspace.
extern "C" int kfamd_attn_chunk_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens,
                                           void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                           int t_bound, float scale, const long long* st, const int* page_table,
                                           long long table_stride, int n_pages, void* stream) {
  if (G <= 0 || !page_table) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Bf16Rows>(q, k_pages, v_pages, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                    scale, st, stream, G, 0, false, page_table, table_stride, n_pages);
}

extern "C" int kfamd_attn_chunk_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const float* k_scale,
                                          const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                          int Hkv, int G, int D, int T, int t_bound, float scale, const long long* st,
                                          const int* page_table, long long table_stride, int n_pages, void* stream) {
  if (G <= 0 || !page_table) return KFAMD_EINVAL;
  return attn_chunk<kfkv::Fp8Rows>(q, k_pages, v_pages, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound,
                                   scale, st, stream, G, 0, false, page_table, table_stride, n_pages);
}
