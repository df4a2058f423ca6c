// attn_kv.hip — attention over a KV cache (split-KV, 1 .. 16 query rows, bf16 or FP8 cache) and the appends.
//
// Tq (1 .. 16) query rows per (batch, head), already appended to the cache [B][H][Tcap][D], attend it
// causally: row i sees keys 0 .. lens[b] - Tq + i. Decode is Tq = 1. The step is a KV stream (one query
// row: no MFMA tile to fill, cdna_hip_programming.md "Attention decode (single-token)"): K and V go
// straight to VGPRs, the dot products and P.V run on the VALU in fp32, and K and V are streamed once per
// (b, h, split) for up to 8 rows — the whole gain of a multi-row call over Tq single-row ones.
//
// Two kernel bodies, both over a row format Fmt (Bf16Rows / Fp8Rows below: the load width, the unpack, the
// unroll, and whether a row carries scales; both formats put 8 elements in a lane, so a key row is D / 8
// lanes wide, and the lane groups, the keys per block step and the accumulators per lane are the same):
//   attn_extend_split<Fmt, D, R>  R row slots, 1 / 2 / 4 / 8: the row count rounded up to a power of two;
//         slots beyond Tq never see a valid key and are never stored. Tq = 9 .. 16 runs two split launches
//         (rows 0 .. 7, rows 8 .. Tq - 1). Sixteen slots (16 x 8 fp32 accumulators next to 16 rows of q)
//         exceed the 256-VGPR budget and spill, so they are not instantiated.
//   attn_decode_split<Fmt, D>  the single-row entry points' kernel: the same arithmetic in the same order as
//         R = 1 with Tq = 1, row0 = 0 (o and lse are bit-identical: tests/test_gpu_attn_kv_unified.py), kept
//         as a body of its own because a graphed single-token step at B*H = 16 is latency-bound and the
//         general body, launched for it, was 1.0 - 1.5 % of a gpt-1b step slower (profiles/attn_kv_unify).
// They share the formats, the split bookkeeping's constants, the host check and the launcher; each has its
// combine (attn_decode_combine is attn_kv_combine at Tq = 1).
// Up to 16 rows this VALU form serves every Tq, no cut-over inside attention_extend. More rows per call
// take the MFMA form, attn_chunk_split in attn_kv_mfma.hip (128-row query tiles on
// v_mfma_f32_32x32x16_bf16, V read transposed from LDS; any Tq, ops.attention_chunk): it shares the row
// formats, kSplitKeys, the split records and attn_kv_combine with this file through attn_kv_rows.h.
//
// Split structure: the key range [0, t_bound) is cut in fixed chunks of kSplitKeys keys; workgroup
// (split, h, b) — 256 threads — walks its chunk. The block's 256 / (D / 8) lane groups take consecutive
// keys, Fmt::unroll(R) keys per group and step, with the next step's loads issued before the current
// step's arithmetic. Each lane group keeps its own fp32 online softmax (m, l, o[8 dims per lane]) per
// row slot; the groups meet in LDS once, at the end. With one split the block writes the bf16 rows
// directly; otherwise it writes (m, l, o[D]) fp32 per row to the workspace ([B][H][Tq][nsplit]) and a
// second small launch (attn_kv_combine) merges the splits in a fixed order: two dependent launches on
// one stream, no cross-workgroup waiting, no atomics, results bitwise repeatable.
//
// lens is DEVICE memory and is never advanced here: a captured step replays while the position advances.
// Keys at or beyond a row's limit are excluded by a branch on the key index, never multiplied by zero:
// the cache there may hold NaN (bf16), or codes 0x7F and NaN scales (FP8). Addresses, the scale loads'
// too, are clamped to a valid key. The causal limit differs per row, so "no key in this split" (m = -inf,
// l = 0, skipped by select in every merge) happens per row, not only per split.
//
// The FP8 cache holds OCP e4m3fn codes [B][H][Tcap][D] (one byte per element) and one fp32 scale per
// stored row ([B][H][Tcap], one tensor for K and one for V). A row x[0..D) of bf16 values read as fp32 is
// stored as
//     scale = max|x| / 448   (1 for an all-zero row),   code = RNE_e4m3(clamp(x / scale, -448, 448)),
// clamped in fp32 before v_cvt_pk_fp8_f32 so that nothing depends on the hardware's FP8 overflow mode;
// code * scale gives the row back. Attention never dequantises to memory: the codes are unpacked to fp32
// on the VALU (v_cvt_pk_f32_fp8, 4 per 8 elements where bf16 takes 8 shifts / ands), the score of key j
// is (q . codes_k[j]) * kscale[j], and vscale[j] is folded into p before the P.V FMAs. The scale of key j
// is loaded with its row (every lane of the group reads the same word) and prefetched with it. A lane
// takes 8 code bytes in one 8-B load; the 16-B form (D / 16 lanes per row) was not built: at D = 64 it
// leaves 4-lane groups, which wave_ops.h's group reductions do not cover, and it doubles the
// accumulators per lane, a certain spill at 8 row slots.
//
// Grouped-query attention (G query heads per K / V head, query head h on K / V head h / G; G in {1, 2, 4, 8,
// 16}): the G heads of a token are more rows on the same K / V stream. The grouped entry points launch
// attn_extend_split<Fmt, D, R, true> on the grid (split, K / V head, b) with the T * G rows of a K / V head
// flattened token-major (RowMap below: r = t * G + g, limit lens[b] - T + r / G, non-decreasing in r, which
// the split launches row0 .. row0 + 7 rely on). The mapping enters the q load, the limit, the o / lse stores;
// the split records are indexed by (b, K / V head, r) and attn_kv_combine_gqa<D> applies the same mapping to
// its store. Routing: T * G <= 16 rows, 1 .. 8 row slots per launch and two launches for 9 .. 16 rows, as
// for plain rows; decode (T = 1) with G > 1 is this body with R = G slots (G = 16: two launches), and
// attn_decode_split stays the G = 1 single-row body. G = 1 through a grouped entry point launches the plain
// kernels. The group size is a kernel argument (lg = log2 G) read only by the GQ = true instantiations: the
// GQ = false ones are the kernels as they were (same registers, o and lse bit-identical to the previous build
// on 186 decode / extend / chunk / append outputs).
// Cut-over (profiles/gqa; D = 128, capacity 4096, B = 8 x 16 query heads, 2048 / 4096 keys, medians of 7
// interleaved blocks, caches rotated): at 8 rows per K / V head (G = 8 decode; G = 4, T = 2; G = 2, T = 4) this
// form takes 26 - 67 us where attn_chunk_split takes 16 - 41 us, 1.5 - 2.0x; at 16 rows (two launches here)
// 46 - 124 us against 16 - 41 us, 2.5 - 3.7x; bf16 and FP8 alike, every case beyond the blocks' spread. 8 row
// slots are VALU-bound, as for plain rows, and the grouped grid has only B * Hkv * nsplit workgroups. So for
// G > 1 ops.attention_decode / attention_extend take this form below 8 rows (G = 2, 4 decode; G = 2, T <= 3)
// and the MFMA form from 8 rows on (ops.decode.GQA_MFMA_MIN_ROWS); G = 1 does not move. The entry points
// here still serve every T * G <= 16. Decode time against G as routed: profiles/gqa/README.md — it does
// not follow the K / V bytes: G = 2 is 1.2 - 1.6x and G = 4 1.1 - 2.1x faster than G = 1 on this form.
//
// Sliding window (the rule: the docstring of ops/decode.py): a row whose causal limit is L (nk[r] below) sees key j
// iff max(0, L - W) <= j < L, W >= 1 a host integer, the same for every row of a call. WIN = true instantiations of
// attn_decode_split and attn_extend_split (plain and GQ), behind the kfamd_attn_*_win_* entry points; the WIN = false
// ones are the kernels as they were (same code, same registers: the table below). The lower bound is computed next
// to the limit from the device-side lens, and a key below it is excluded exactly as a key at or beyond the limit is,
// by the branch on the key index: the cache outside every row's window may hold NaN or 0x7F codes and NaN scales,
// and addresses stay clamped to a valid key. The grid still comes from t_bound (lens stays on the device, the launch
// stays capturable); a workgroup whose whole split lies below the lowest lower bound of its rows (the launch's first
// row's: the limits are non-decreasing) writes the empty record and returns before any K / V load — the merges skip
// that record by select, and with one split the case cannot arise (the lower bound lies below lens) — and the first
// live split starts its walk at the block step that holds the lower bound, loads ahead of arithmetic as before.
// W >= t_bound can remove no key: the launcher then runs the WIN = false kernels. Every WIN = true instantiation uses
// the VGPRs of its WIN = false twin in the table below (66 / 84 decode; 64 / 92 / 129 / 201 and 84 / 112 / 149 / 197
// extend, GQ alike), scratch 0. Measured: profiles/window.
//
// Ring-buffer cache (the rule: the docstring of ops/decode.py): key j lives in slot j % C, C a multiple of kSplitKeys,
// lens absolute and unbounded. RING = true instantiations of attn_decode_split and attn_extend_split (plain and GQ, all
// row slots; RING implies WIN), behind the kfamd_attn_*_ring_* entry points; the RING = false ones are the kernels as
// they were (the 103 kernels of this file, attn_kv_mfma.hip and rope_bf16.hip compared as ISA with the previous build:
// identical). The grid is ceil((W + T - 1) / 256) + 1 splits per (b, h), a function of W and T alone; split s of batch
// row b covers absolute keys from base_b + 256 s on, base_b = (max(lens[b] - T + 1 - W, 0) / 256) * 256 computed on the
// device, so the partition stays the absolute 256-aligned one and every early return stays block-uniform. A split is
// one contiguous run of slots: its slot base comes once per workgroup from the scalar k0 % C and is folded into the
// K / V / scale pointers, the in-split addressing stays key - k0, and the look-ahead address is clamped as an absolute
// key index (min(key, last)) before it is mapped to the slot. No key index is ever multiplied by a stride. Slots
// outside every row's window, those after key lens[b] - 1 included, are excluded by the key index and may hold NaN.
// VGPRs: those of the WIN twins in the table below (66 / 84 decode; 64 / 92 / 129 / 201 and 84 / 112 / 149 / 197
// extend, GQ alike), scratch 0. kv_append<true> / kv_append_fp8<D, true> write slot (lens[b] + t) % C: 20 / 32 (D = 64), 31 (D = 128) VGPRs.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): VGPRs, the same
// at D = 64 and at D = 128 unless two are given; scratch is 0 for every instantiation. "before": the four
// kernels this file replaced, D = 64 / 128.
//   instantiation                      VGPRs   before
//   attn_decode_split<Bf16Rows, D>       66    66 /  66
//   attn_decode_split<Fp8Rows, D>        84    84 /  84
//   attn_extend_split<Bf16Rows, D, 1>    64    72 /  67
//   attn_extend_split<Bf16Rows, D, 2>    92    96 /  96
//   attn_extend_split<Bf16Rows, D, 4>   129   130 / 130
//   attn_extend_split<Bf16Rows, D, 8>   201   202 / 202
//   attn_extend_split<Fp8Rows, D, 1>     84    97 /  84
//   attn_extend_split<Fp8Rows, D, 2>    112   116 / 116
//   attn_extend_split<Fp8Rows, D, 4>    149   150 / 150
//   attn_extend_split<Fp8Rows, D, 8>    197   198 / 198
//   kv_append / kv_append_fp8<D>     21 / 39   21 /  39
// RING = true (kfamd_attn_*_ring_*, kfamd_kv_append_ring_*), D = 64 / 128 alike unless two are given, GQ alike, scratch 0:
//   attn_decode_split<Bf16Rows, D, true, true>             66
//   attn_decode_split<Fp8Rows, D, true, true>              84
//   attn_extend_split<Bf16Rows, D, 1, GQ, true, true>      64
//   attn_extend_split<Bf16Rows, D, 2, GQ, true, true>      92
//   attn_extend_split<Bf16Rows, D, 4, GQ, true, true>     129
//   attn_extend_split<Bf16Rows, D, 8, GQ, true, true>     201
//   attn_extend_split<Fp8Rows, D, 1, GQ, true, true>       84
//   attn_extend_split<Fp8Rows, D, 2, GQ, true, true>      112
//   attn_extend_split<Fp8Rows, D, 4, GQ, true, true>      149
//   attn_extend_split<Fp8Rows, D, 8, GQ, true, true>      197
//   kv_append<true>                                        20
//   kv_append_fp8<D, true>                            32 / 31
// PAGED = true (a paged cache, kfamd_attn_*_paged_*, kfamd_kv_append_paged_*; the rule: the docstring of ops/decode.py):
// the flat set only, PAGED combines with neither WIN nor RING. A live workgroup reads its split's one page id as a
// block-uniform scalar after the empty-split return (an absent entry is never dereferenced), clamps it into
// [0, n_pages - 1], forms the K / V / scale bases from pool + page * page_stride + h * kh and indexes by key - k0 as the
// RING branch does. Same partition, same order, same arithmetic: o and lse equal the flat launch's bit for bit
// (tests/test_gpu_paged.py). VGPRs, D = 64 / 128 and GQ alike, scratch 0; the pre-existing 154 kernels of this file,
// attn_kv_mfma.hip and rope_bf16.hip compared as ISA with the previous build: identical.
//   attn_decode_split<Bf16Rows, D, false, false, true>            66
//   attn_decode_split<Fp8Rows, D, false, false, true>             84
//   attn_extend_split<Bf16Rows, D, 1 / 2 / 4 / 8, GQ, false, false, true>    64 /  92 / 129 / 201
//   attn_extend_split<Fp8Rows, D, 1 / 2 / 4 / 8, GQ, false, false, true>     84 / 112 / 149 / 197
//   kv_append_paged                                               20
//   kv_append_fp8_paged<D>                                        37
// The comparison with the previous build and these counts: tools/kernel_isa_diff.py (two directories of hipcc -S output).
// The GQ = true instantiations of attn_extend_split use the same VGPRs as the GQ = false rows above, R for R
// (64 / 92 / 129 / 201 and 84 / 112 / 149 / 197), the same LDS, scratch 0; attn_kv_combine<D> and
// attn_kv_combine_gqa<D> 12 VGPRs each.
// The extend body's LDS merge is written as one pass and, for R = 8, a guarded second one: as a loop over
// the passes with an early exit it cost R = 1 up to 13 VGPRs (Fp8Rows, D = 64: 97, one wave per SIMD less).
// Measured (profiles/decode, profiles/extend, profiles/kv_fp8, profiles/attn_kv_unify; D = 128, capacity
// 4096): a multi-row call against Tq single-row calls is 1.7-2.3x at Tq = 2, 2.8-4.5x at 4, 3.4-7.0x at 8,
// 3.5-7.5x at 16; up to Tq = 4 it stays a KV stream (4.0-4.5 TB/s at B*H = 128, >= 2048 keys), at Tq = 8
// the VALU work sets the time and Tq = 16 costs twice Tq = 8. FP8 against bf16: decode 1.57-1.71x faster
// at B*H = 128 with 2048 / 4096 keys; Tq = 4 1.17x at 2048 keys and a tie at 4096; Tq = 8 ties or loses
// 4 %; ties within the launch floor at 128 keys and at B*H = 16. The FP8 append is 1.33x slower than the
// bf16 copy at T = 2048 (8 IEEE divisions per lane): 63 us per layer of a 2048-token prefill.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "attn_kv_rows.h"
#include "kfamd_kernels.h"
#include "wave_ops.h"

namespace {

using namespace kfkv;  // the row formats (Bf16Rows, Fp8Rows), kSplitKeys and the host checks: attn_kv_rows.h

constexpr int kThreads = 256;
constexpr int kMaxRows = 16;
constexpr int kSlotRows = 8;   // query rows per split launch (16 row slots spill: see the header)
constexpr int kMergeRows = 4;  // row slots merged per LDS pass

// ---- attention ---------------------------------------------------------------------------------
struct AttnArgs {
  const __bf16* q;
  const void* k;  // Fmt::Elem
  const void* v;
  const float* ks;  // Fmt::kScaled only, as ksb .. vsh
  const float* vs;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int B, H, Tq, row0, t_bound, nsplit;  // a split launch holds rows row0 .. row0 + R - 1 of the Tq
  float scale_log2;
  int lg;  // GQ kernels only: log2 of the group size G. H is then Hkv and Tq the T * G flattened rows
  long long qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh, ksb, ksh, vsb, vsh;
  int window;  // WIN kernels only: the sliding window W >= 1 (the rule: the header)
  int cap;     // RING kernels only: the ring's capacity C, a multiple of kSplitKeys
};

// The single-row kernel's arguments: AttnArgs without Tq, row0 and the t strides.
struct DecodeArgs {
  const __bf16* q;
  const void* k;
  const void* v;
  const int* lens;
  __bf16* o;
  float* lse;
  float* ws;
  int B, H, t_bound, nsplit;
  float scale_log2;
  long long qb, qh, kb, kh, kt, vb, vh, vt, ob, oh;
  const float* ks;  // Fmt::kScaled only, as ksb .. vsh
  const float* vs;
  long long ksb, ksh, vsb, vsh;
  int window;  // WIN kernel only
  int cap;     // RING kernel only
};

// PAGED kernels (the page rule: the docstring of ops/decode.py): the flat arguments, with the page stride of K, V and
// the scales in kb, vb, ksb, vsb, plus the page table. Types of their own, so that the flat kernels' argument blocks
// (and with them their code) stay as they were.
struct PagedAttnArgs : AttnArgs {
  const int* pt;  // device int32 [B][pts]: the page of keys 256 c .. 256 c + 255 of row b, -1 for none
  long long pts;
  int n_pages;
};
struct PagedDecodeArgs : DecodeArgs {
  const int* pt;
  long long pts;
  int n_pages;
};

// A page id read from the table, for a LOAD: clamped into [0, n_pages - 1] whatever the table holds.
__device__ __forceinline__ int load_page(const int* pt, long long at, int n_pages) {
  return min(max(pt[at], 0), n_pages - 1);
}

// One query row per (b, h). workspace: [B][H][nsplit][2] (m, l) then [B][H][nsplit][D] (o), fp32: the
// extend kernel's at Tq = 1. What the extend body's comments say about key validity, clamped addresses,
// the block-uniform early return, whole block steps and the window's lower bound holds here word for word.
template <class Fmt, int D, bool WIN, bool RING, bool PAGED>
__global__ __launch_bounds__(kThreads) void attn_decode_split(std::conditional_t<PAGED, PagedDecodeArgs, DecodeArgs> a) {
  static_assert(WIN || !RING, "a ring always has a window");
  static_assert(!PAGED || !WIN, "a paged cache has neither a window nor a ring");
  typedef typename Fmt::Elem Elem;
  typedef typename Fmt::Vec Vec;
  constexpr int kUnroll = Fmt::unroll(1);
  constexpr int G = D / 8;             // lanes per key row
  constexpr int NG = kThreads / G;     // lane groups per block (= keys per block and unroll slot)
  constexpr int KSTEP = NG * kUnroll;  // keys per block step
  static_assert(kSplitKeys % KSTEP == 0, "a split holds a whole number of block steps");
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int grp = tid / G, piece = tid % G;

  __shared__ float s_m[NG], s_l[NG];
  __shared__ float s_o[NG][D + 4];

  int len = a.lens[b];
  if constexpr (RING) len = max(len, 0);  // absolute, not bounded by the capacity
  else len = len < 0 ? 0 : (len > a.t_bound ? a.t_bound : len);
  int k0 = split * kSplitKeys;
  if constexpr (RING) k0 += max(len - a.window, 0) / kSplitKeys * kSplitKeys;  // + base_b: the split that holds lo
  const int k1 = min(k0 + kSplitKeys, len);  // valid keys of this split: [k0, k1)
  int lo = 0;  // WIN: the row sees keys [lo, len)
  if constexpr (WIN) lo = max(len - a.window, 0);
  const long long bh = ((long long)b * a.H + h);
  float* ws_ml = a.ws + (bh * a.nsplit + split) * 2;
  float* ws_o = a.ws + (long long)a.B * a.H * a.nsplit * 2 + (bh * a.nsplit + split) * D;

  if (k1 <= k0 || (WIN && lo >= k1)) {  // empty split (only reachable with nsplit > 1 or len == 0), or one below the window
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
  Bf16Rows::unpack8(*reinterpret_cast<const u32x4*>(a.q + b * a.qb + h * a.qh + piece * 8), qf);
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[i] *= a.scale_log2;

  // PAGED: the split's 256 keys are one page, its id a block-uniform scalar read after the early return above (an
  // absent entry is never dereferenced) and clamped; kb, vb, ksb, vsb are then the page strides
  long long sl = b;  // the slice of the cache's first dimension
  if constexpr (PAGED) sl = load_page(a.pt, b * a.pts + k0 / kSplitKeys, a.n_pages);
  const Elem* kbase = static_cast<const Elem*>(a.k) + sl * a.kb + h * a.kh + piece * 8;
  const Elem* vbase = static_cast<const Elem*>(a.v) + sl * a.vb + h * a.vh + piece * 8;
  const float *ksbase = nullptr, *vsbase = nullptr;
  if constexpr (Fmt::kScaled) {
    ksbase = a.ks + sl * a.ksb + h * a.ksh;
    vsbase = a.vs + sl * a.vsb + h * a.vsh;
  }
  if constexpr (RING) {  // the split's 256 keys are one run of slots from k0 % C on: what follows indexes it by key - k0
    const int s0 = k0 % a.cap;
    kbase += s0 * a.kt;
    vbase += s0 * a.vt;
    if constexpr (Fmt::kScaled) ksbase += s0, vsbase += s0;
  }
  const int last = k1 - 1;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  Vec kn[kUnroll], vn[kUnroll];
  float ksn[kUnroll], vsn[kUnroll];  // Fmt::kScaled only
  auto load_ahead = [&](int u, int key) {
    key = min(key, last);
    if constexpr (RING || PAGED) key -= k0;  // clamped as an absolute index, then mapped to the slot (the page's row)
    kn[u] = *reinterpret_cast<const Vec*>(kbase + key * a.kt);
    vn[u] = *reinterpret_cast<const Vec*>(vbase + key * a.vt);
    if constexpr (Fmt::kScaled) {
      ksn[u] = ksbase[key];
      vsn[u] = vsbase[key];
    }
  };
  int kbeg = k0;  // WIN: the block step that holds the first key of the window
  if constexpr (WIN) kbeg = k0 + max(lo - k0, 0) / KSTEP * KSTEP;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) load_ahead(u, kbeg + u * NG + grp);
  for (int kk = kbeg; kk < k1; kk += KSTEP) {
    Vec kc[kUnroll], vc[kUnroll];
    float ksc[kUnroll], vsc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      kc[u] = kn[u];
      vc[u] = vn[u];
      if constexpr (Fmt::kScaled) {
        ksc[u] = ksn[u];
        vsc[u] = vsn[u];
      }
    }
    if (kk + KSTEP < k1) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) load_ahead(u, kk + KSTEP + u * NG + grp);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int key = kk + u * NG + grp;
      float kf[8];
      Fmt::unpack8(kc[u], kf);
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) part = fmaf(qf[i], kf[i], part);
      float s = kfw::group_sum<G>(part);
      if constexpr (Fmt::kScaled) s *= ksc[u];
      if (key < k1 && (!WIN || key >= lo)) {
        float vf[8];
        Fmt::unpack8(vc[u], vf);
        const float mn = fmaxf(m, s);
        const float corr = exp2f(m - mn);
        float p = exp2f(s - mn);
        l = l * corr + p;
        if constexpr (Fmt::kScaled) p *= vsc[u];
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
// Where row r of the Tq rows of (b, h) lives. Plain (GQ = false): row r is token r of head h. Grouped
// (GQ = true): h is a K / V head, the rows are the T * G (token, head-in-group) pairs flattened token-major,
// r = t * G + g: token r >> lg of query head (h << lg) + (r & (G - 1)), which attends keys
// 0 .. len - T + (r >> lg) — non-decreasing in r, as the split launches row0 .. row0 + 7 assume.
template <bool GQ>
struct RowMap {
  int lg, T, Hq, h0;
  __device__ __forceinline__ RowMap(int lg_, int Tq, int H, int h)
      : lg(GQ ? lg_ : 0), T(Tq >> lg), Hq(H << lg), h0(h << lg) {}
  __device__ __forceinline__ int tok(int r) const { return r >> lg; }
  __device__ __forceinline__ int head(int r) const { return h0 + (r & ((1 << lg) - 1)); }
};

// workspace: [B][H][Tq][nsplit][2] (m, l) then [B][H][Tq][nsplit][D] (o), fp32
// WIN: row slot r sees keys [lo[r], nk[r]) only, lo = max(0, nk - window); a key below lo is excluded as one at or
// beyond nk is, by the branch on the key index. The limits are non-decreasing in r, so the launch's first row has
// its lowest lower bound: a split that ends at or below it holds no key for any row, and inside the first live split
// the walk starts at the block step that holds it.
template <class Fmt, int D, int R, bool GQ, bool WIN, bool RING, bool PAGED>
__global__ __launch_bounds__(kThreads) void attn_extend_split(std::conditional_t<PAGED, PagedAttnArgs, AttnArgs> a) {
  static_assert(WIN || !RING, "a ring always has a window");
  static_assert(!PAGED || !WIN, "a paged cache has neither a window nor a ring");
  typedef typename Fmt::Elem Elem;
  typedef typename Fmt::Vec Vec;
  constexpr int kUnroll = Fmt::unroll(R);
  constexpr int G = D / 8;             // lanes per key row
  constexpr int NG = kThreads / G;     // lane groups per block
  constexpr int KSTEP = NG * kUnroll;  // keys per block step
  constexpr int RC = R < kMergeRows ? R : kMergeRows;
  // a block step never reaches into the next split: `key < nk[r]` alone then decides a key's validity
  static_assert(kSplitKeys % KSTEP == 0, "a split holds a whole number of block steps");
  static_assert(R <= 2 * RC, "the LDS merge takes one or two passes");
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int grp = tid / G, piece = tid % G;
  const int Tq = a.Tq, row0 = a.row0;
  const RowMap<GQ> rm(a.lg, Tq, a.H, h);

  __shared__ float s_m[NG][RC], s_l[NG][RC];
  __shared__ float s_o[NG][RC][D + 4];

  int len = a.lens[b];
  if constexpr (RING) len = max(len, 0);  // absolute, not bounded by the capacity
  else len = len < 0 ? 0 : (len > a.t_bound ? a.t_bound : len);
  int k0 = split * kSplitKeys;
  // + base_b, from the call's first token (the same for the launches of rows 0 .. 7 and 8 .. 15)
  if constexpr (RING) k0 += max(len - rm.T + 1 - a.window, 0) / kSplitKeys * kSplitKeys;
  const int k1 = min(k0 + kSplitKeys, len);  // keys of this split that the last row may see: [k0, k1)
  const long long bh = (long long)b * a.H + h;
  const long long nrows = (long long)a.B * a.H * Tq;
  int blo = 0;  // WIN: the lowest lower bound of the launch's rows, its first row's
  if constexpr (WIN) blo = max(len - rm.T + rm.tok(row0) + 1 - a.window, 0);

  if (k1 <= k0 || (WIN && blo >= k1)) {  // empty split for every row (block-uniform, before any barrier)
    for (int r = row0; r < min(row0 + R, Tq); ++r) {
      const long long row = bh * Tq + r;
      if (a.nsplit > 1) {
        if (tid == 0) {
          a.ws[(row * a.nsplit + split) * 2] = -INFINITY;
          a.ws[(row * a.nsplit + split) * 2 + 1] = 0.f;
        }
        if (tid < D) a.ws[nrows * a.nsplit * 2 + (row * a.nsplit + split) * D + tid] = 0.f;
      } else {
        if (tid < D) a.o[b * a.ob + rm.tok(r) * a.ot + rm.head(r) * a.oh + tid] = (__bf16)0.f;
        if (tid == 0 && a.lse) a.lse[((long long)b * rm.T + rm.tok(r)) * rm.Hq + rm.head(r)] = -INFINITY;
      }
    }
    return;
  }

  // row slot r sees keys [0, nk[r]); a padding slot (r >= Tq) and a row before the sequence's start see none
  float qf[R][8];
  int nk[R];
  int lo[R];  // WIN only
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gr = row0 + r;               // the slot's row of the Tq
    const int rr = gr < Tq ? gr : Tq - 1;  // padding slots read a valid row
    Bf16Rows::unpack8(
        *reinterpret_cast<const u32x4*>(a.q + b * a.qb + rm.tok(rr) * a.qt + rm.head(rr) * a.qh + piece * 8), qf[r]);
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[r][i] *= a.scale_log2;
    nk[r] = gr < Tq ? len - rm.T + rm.tok(gr) + 1 : 0;
    if constexpr (WIN) lo[r] = max(nk[r] - a.window, 0);
  }

  // PAGED: the split's 256 keys are one page, its id a block-uniform scalar read after the early return above (an
  // absent entry is never dereferenced) and clamped; kb, vb, ksb, vsb are then the page strides
  long long sl = b;  // the slice of the cache's first dimension
  if constexpr (PAGED) sl = load_page(a.pt, b * a.pts + k0 / kSplitKeys, a.n_pages);
  const Elem* kbase = static_cast<const Elem*>(a.k) + sl * a.kb + h * a.kh + piece * 8;
  const Elem* vbase = static_cast<const Elem*>(a.v) + sl * a.vb + h * a.vh + piece * 8;
  const float *ksbase = nullptr, *vsbase = nullptr;
  if constexpr (Fmt::kScaled) {
    ksbase = a.ks + sl * a.ksb + h * a.ksh;
    vsbase = a.vs + sl * a.vsb + h * a.vsh;
  }
  if constexpr (RING) {  // the split's 256 keys are one run of slots from k0 % C on: what follows indexes it by key - k0
    const int s0 = k0 % a.cap;
    kbase += s0 * a.kt;
    vbase += s0 * a.vt;
    if constexpr (Fmt::kScaled) ksbase += s0, vsbase += s0;
  }
  const int last = k1 - 1;  // addresses are clamped to a valid key; the key index decides validity

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }

  Vec kn[kUnroll], vn[kUnroll];
  float ksn[kUnroll], vsn[kUnroll];  // Fmt::kScaled only
  auto load_ahead = [&](int u, int key) {
    key = min(key, last);
    if constexpr (RING || PAGED) key -= k0;  // clamped as an absolute index, then mapped to the slot (the page's row)
    kn[u] = *reinterpret_cast<const Vec*>(kbase + key * a.kt);
    vn[u] = *reinterpret_cast<const Vec*>(vbase + key * a.vt);
    if constexpr (Fmt::kScaled) {
      ksn[u] = ksbase[key];
      vsn[u] = vsbase[key];
    }
  };
  int kbeg = k0;  // WIN: the block step that holds the lowest lower bound
  if constexpr (WIN) kbeg = k0 + max(blo - k0, 0) / KSTEP * KSTEP;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) load_ahead(u, kbeg + u * NG + grp);
  for (int kk = kbeg; kk < k1; kk += KSTEP) {
    Vec kc[kUnroll], vc[kUnroll];
    float ksc[kUnroll], vsc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      kc[u] = kn[u];
      vc[u] = vn[u];
      if constexpr (Fmt::kScaled) {
        ksc[u] = ksn[u];
        vsc[u] = vsn[u];
      }
    }
    if (kk + KSTEP < k1) {  // the next step's loads go out before this step's arithmetic
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) load_ahead(u, kk + KSTEP + u * NG + grp);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int key = kk + u * NG + grp;
      float kf[8], vf[8];
      Fmt::unpack8(kc[u], kf);
      Fmt::unpack8(vc[u], vf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) part = fmaf(qf[r][i], kf[i], part);
        float s = kfw::group_sum<G>(part);  // every lane of the group: scale * log2e * q_r.k
        if constexpr (Fmt::kScaled) s *= ksc[u];
        bool seen = key < nk[r];  // group-uniform; an invalid key touches no state
        if constexpr (WIN) seen = seen && key >= lo[r];
        if (seen) {
          const float mn = fmaxf(m[r], s);
          const float corr = exp2f(m[r] - mn);  // m = -inf on the first key: exp2(-inf) = 0
          float p = exp2f(s - mn);
          l[r] = l[r] * corr + p;
          if constexpr (Fmt::kScaled) p *= vsc[u];  // V's scale folded into p
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(acc[r][i], corr, p * vf[i]);
          m[r] = mn;
        }
      }
    }
  }

  // the block's lane groups meet in LDS, RC row slots per pass
  auto merge_pass = [&](const int r0) {
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
      const int r = row0 + r0 + j;
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
        a.o[b * a.ob + rm.tok(r) * a.ot + rm.head(r) * a.oh + d] = (__bf16)(any ? O / L : 0.f);
        if (d == 0 && a.lse)
          a.lse[((long long)b * rm.T + rm.tok(r)) * rm.Hq + rm.head(r)] = any ? (M + log2f(L)) * kLn2 : -INFINITY;
      }
    }
  };
  merge_pass(0);
  if constexpr (R > RC) {
    if (row0 + RC < Tq) {  // block-uniform: otherwise only padding slots are left
      __syncthreads();     // the first pass has been read
      merge_pass(RC);
    }
  }
}

// The merge of the splits' per-row (m, l, o[D]) fp32 records into bf16 rows: reads only the workspace.
// B is an argument, not gridDim.y: the launch dimensions are read from beyond the 64 bytes of arguments,
// one more serial scalar-load miss per call of a kernel that runs for a few microseconds.
template <int D, bool GQ>
__device__ __forceinline__ void kv_combine_row(const float* __restrict__ ws, __bf16* __restrict__ o,
                                               float* __restrict__ lse, int B, int H, int Tq, int nsplit, long long ob,
                                               long long ot, long long oh, int lg) {
  const int h = blockIdx.x, b = blockIdx.y, r = blockIdx.z, d = threadIdx.x;
  const RowMap<GQ> rm(lg, Tq, H, h);
  const long long nrows = (long long)B * H * Tq;
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
  o[b * ob + rm.tok(r) * ot + rm.head(r) * oh + d] = (__bf16)(any ? O / L : 0.f);
  if (d == 0 && lse)
    lse[((long long)b * rm.T + rm.tok(r)) * rm.Hq + rm.head(r)] = any ? (M + log2f(L)) * kLn2 : -INFINITY;
}

template <int D>
__global__ __launch_bounds__(D) void attn_kv_combine(const float* __restrict__ ws, __bf16* __restrict__ o,
                                                     float* __restrict__ lse, int B, int H, int Tq, int nsplit,
                                                     long long ob, long long ot, long long oh) {
  kv_combine_row<D, false>(ws, o, lse, B, H, Tq, nsplit, ob, ot, oh, 0);
}

// The grouped form (RowMap<true>): H is Hkv, Tq the T * G flattened rows. A kernel of its own: the plain
// one's arguments end at 64 bytes (above).
template <int D>
__global__ __launch_bounds__(D) void attn_kv_combine_gqa(const float* __restrict__ ws, __bf16* __restrict__ o,
                                                         float* __restrict__ lse, int B, int H, int Tq, int nsplit,
                                                         long long ob, long long ot, long long oh, int lg) {
  kv_combine_row<D, true>(ws, o, lse, B, H, Tq, nsplit, ob, ot, oh, lg);
}

// The same merge for the single-row kernel's records (Tq = 1, no t stride), kept next to it for the reason
// given in the header: through attn_kv_combine a graphed single-token step measured 0.1 - 0.2 us per call
// slower at B*H = 16.
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

template <class Fmt, int D, bool GQ, bool WIN, bool RING, bool PAGED = false, class Args = AttnArgs>
void launch_rows(const Args& a, int n, dim3 grid, hipStream_t s) {  // n: rows of this launch, 1 .. kSlotRows
  const dim3 block(kThreads);
  if (n == 1) hipLaunchKernelGGL((attn_extend_split<Fmt, D, 1, GQ, WIN, RING, PAGED>), grid, block, 0, s, a);
  else if (n == 2) hipLaunchKernelGGL((attn_extend_split<Fmt, D, 2, GQ, WIN, RING, PAGED>), grid, block, 0, s, a);
  else if (n <= 4) hipLaunchKernelGGL((attn_extend_split<Fmt, D, 4, GQ, WIN, RING, PAGED>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((attn_extend_split<Fmt, D, 8, GQ, WIN, RING, PAGED>), grid, block, 0, s, a);
}

template <class Fmt, int D, bool WIN, bool RING>
void launch_group(const AttnArgs& a, int n, dim3 grid, hipStream_t s) {
  if (a.lg > 0) launch_rows<Fmt, D, true, WIN, RING>(a, n, grid, s);  // G = 1 through a grouped entry point: the plain kernels
  else launch_rows<Fmt, D, false, WIN, RING>(a, n, grid, s);
}

template <class Fmt, int D>
void launch_split(const AttnArgs& a, int n, dim3 grid, hipStream_t s) {
  if (a.cap > 0) launch_group<Fmt, D, true, true>(a, n, grid, s);
  else if (a.window > 0) launch_group<Fmt, D, true, false>(a, n, grid, s);
  else launch_group<Fmt, D, false, false>(a, n, grid, s);
}

// a paged cache: the flat set only (neither WIN nor RING)
template <class Fmt, int D>
void launch_split(const PagedAttnArgs& a, int n, dim3 grid, hipStream_t s) {
  if (a.lg > 0) launch_rows<Fmt, D, true, false, false, true>(a, n, grid, s);
  else launch_rows<Fmt, D, false, false, false, true>(a, n, grid, s);
}

template <class Fmt, int D>
void launch_decode(const DecodeArgs& d, dim3 grid, hipStream_t s) {
  if (d.cap > 0) hipLaunchKernelGGL((attn_decode_split<Fmt, D, true, true, false>), grid, dim3(kThreads), 0, s, d);
  else if (d.window > 0)
    hipLaunchKernelGGL((attn_decode_split<Fmt, D, true, false, false>), grid, dim3(kThreads), 0, s, d);
  else hipLaunchKernelGGL((attn_decode_split<Fmt, D, false, false, false>), grid, dim3(kThreads), 0, s, d);
}

template <class Fmt, int D>
void launch_decode(const PagedDecodeArgs& d, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((attn_decode_split<Fmt, D, false, false, true>), grid, dim3(kThreads), 0, s, d);
}

// Splits of a ring launch: the absolute 256-aligned partition rebased per batch row at base_b = the split that holds
// the first token's lower bound. The rows of a call see at most W + T - 1 keys from there on, which begin up to 255
// keys into their split: ceil((W + T - 1) / 256) + 1 splits always suffice, whatever the position.
int ring_splits(int window, int T) { return (int)(((long long)window + T - 1 + kSplitKeys - 1) / kSplitKeys) + 1; }

// The one launcher behind the four attention entry points. st: the entry point's stride array, q (b, [t,]
// h), k (b, h, t), v (b, h, t), o (b, [t,] h), then for a scaled format k_scale (b, h), v_scale (b, h);
// has_t: the t strides are present. Without them it is a single-row entry point (Tq = 1), which launches
// attn_decode_split. The grouped entry points pass G > 0: H is then Hkv, Tq the token count T, the q / o
// strides' h runs over the Hkv * G query heads, and the kernels see T * G rows per (b, K / V head); G = 1
// there launches what the plain entry points launch. Every KFAMD_EINVAL condition is tested before any
// KFAMD_EALIGN one. window: 0 for the entry points without one, else W >= 1 (the windowed entry points): the WIN
// kernels, except that W >= t_bound can remove no key (lens is clamped to t_bound) and launches the kernels
// without a window.
template <class Fmt>
int attn_kv(const void* q, const void* k, const void* v, const float* ks, const float* vs, const int* lens, void* o,
            float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale, const long long* st,
            bool has_t, void* stream, int G = 0, int window = 0, bool ring = false, const int* pt = nullptr,
            long long pts = 0, int n_pages = 0) {
  if (!q || !k || !v || !lens || !o || !st || B <= 0 || H <= 0 || B > 65535 || H > 65535) return KFAMD_EINVAL;
  if (window < 0) return KFAMD_EINVAL;
  // paged (pt given; the page rule: ops/decode.py): the b strides are page strides, the table holds a column for
  // every split of t_bound, and neither a window nor a ring goes with it
  if (pt && (n_pages < 1 || window > 0 || ring || t_bound < 1 || pts < (t_bound + kSplitKeys - 1) / kSplitKeys))
    return KFAMD_EINVAL;
  // ring: t_bound is the capacity C. W + T - 1 <= C: the step's appends overwrite nothing its first row sees
  if (ring && (window < 1 || t_bound < 1 || t_bound % kSplitKeys || Tq < 1 || (long long)window + Tq - 1 > t_bound))
    return KFAMD_EINVAL;
  const int ring_nsplit = ring ? ring_splits(window, Tq) : 0;
  if (Fmt::kScaled && (!ks || !vs)) return KFAMD_EINVAL;
  const int lg = G > 0 ? group_log2(G) : 0;
  if (lg < 0 || Tq < 1 || Tq > (kMaxRows >> lg)) return KFAMD_EINVAL;
  Tq <<= lg;  // rows per (b, K / V head) from here on
  if ((D != 64 && D != 128) || t_bound < 1) return KFAMD_EINVAL;
  AttnArgs a = {};
  a.qb = *st++, a.qt = has_t ? *st++ : 0, a.qh = *st++;
  a.kb = *st++, a.kh = *st++, a.kt = *st++, a.vb = *st++, a.vh = *st++, a.vt = *st++;
  a.ob = *st++, a.ot = has_t ? *st++ : 0, a.oh = *st++;
  if (Fmt::kScaled) a.ksb = *st++, a.ksh = *st++, a.vsb = *st++, a.vsh = *st++;
  if (a.kt < D || a.vt < D) return KFAMD_EINVAL;
  const long long lim = (1ll << 31) / (long long)sizeof(typename Fmt::Elem);  // a (b, h) slice stays below 2^31 bytes
  if ((long long)t_bound * a.kt >= lim || (long long)t_bound * a.vt >= lim) return KFAMD_EINVAL;
  a.nsplit = ring ? ring_nsplit : (t_bound + kSplitKeys - 1) / kSplitKeys;
  if (a.nsplit > 1 && !ws) return KFAMD_EINVAL;
  if (pt && (kSplitKeys * a.kt >= lim || kSplitKeys * a.vt >= lim)) return KFAMD_EINVAL;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(o) || (ws && !al16(ws))) return KFAMD_EALIGN;
  if (Fmt::kScaled && (!al4(ks) || !al4(vs))) return KFAMD_EALIGN;
  if (pt && !al4(pt)) return KFAMD_EALIGN;
  if ((a.qb | a.qt | a.qh | a.ob | a.ot | a.oh) & 7) return KFAMD_EALIGN;
  if ((a.kb | a.kh | a.kt | a.vb | a.vh | a.vt) & (Fmt::kStrideAlign - 1)) return KFAMD_EALIGN;
  a.q = static_cast<const __bf16*>(q);
  a.k = k, a.v = v, a.ks = ks, a.vs = vs, a.lens = lens;
  a.o = static_cast<__bf16*>(o);
  a.lse = lse;
  a.ws = static_cast<float*>(ws);
  a.B = B, a.H = H, a.Tq = Tq, a.t_bound = t_bound, a.lg = lg;
  a.window = ring ? window : window >= t_bound ? 0 : window;
  a.cap = ring ? t_bound : 0;
  a.scale_log2 = scale * kLog2e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)a.nsplit, (unsigned)H, (unsigned)B);
  if (!has_t) {
    const DecodeArgs d = {a.q,  a.k,  a.v,  a.lens, a.o,  a.lse, a.ws, B,    H,    t_bound, a.nsplit, a.scale_log2,
                          a.qb, a.qh, a.kb, a.kh,   a.kt, a.vb,  a.vh, a.vt, a.ob, a.oh,    a.ks,     a.vs,
                          a.ksb, a.ksh, a.vsb, a.vsh, a.window, a.cap};
    if (pt) {
      PagedDecodeArgs pd = {};
      static_cast<DecodeArgs&>(pd) = d;
      pd.pt = pt, pd.pts = pts, pd.n_pages = n_pages;
      if (D == 64) launch_decode<Fmt, 64>(pd, grid, s);
      else launch_decode<Fmt, 128>(pd, grid, s);
    } else if (D == 64) {
      launch_decode<Fmt, 64>(d, grid, s);
    } else {
      launch_decode<Fmt, 128>(d, grid, s);
    }
  }
  for (a.row0 = 0; has_t && a.row0 < Tq; a.row0 += kSlotRows) {  // one K / V stream per kSlotRows query rows
    const int n = Tq - a.row0 < kSlotRows ? Tq - a.row0 : kSlotRows;
    if (pt) {
      PagedAttnArgs pa = {};
      static_cast<AttnArgs&>(pa) = a;
      pa.pt = pt, pa.pts = pts, pa.n_pages = n_pages;
      if (D == 64) launch_split<Fmt, 64>(pa, n, grid, s);
      else launch_split<Fmt, 128>(pa, n, grid, s);
    } else if (D == 64) {
      launch_split<Fmt, 64>(a, n, grid, s);
    } else {
      launch_split<Fmt, 128>(a, n, grid, s);
    }
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (a.nsplit > 1 && !has_t) {
    const dim3 cgrid((unsigned)H, (unsigned)B);
    if (D == 64)
      hipLaunchKernelGGL(attn_decode_combine<64>, cgrid, dim3(64), 0, s, a.ws, a.o, lse, H, a.nsplit, a.ob, a.oh);
    else
      hipLaunchKernelGGL(attn_decode_combine<128>, cgrid, dim3(128), 0, s, a.ws, a.o, lse, H, a.nsplit, a.ob, a.oh);
    e = hipGetLastError();
  } else if (a.nsplit > 1) {
    e = launch_kv_combine(D, a.ws, a.o, lse, B, H, Tq, a.nsplit, a.ob, a.ot, a.oh, s, lg);
  }
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

// ---- append ------------------------------------------------------------------------------------
// RING (both append kernels): row lens[b] + t goes to slot (lens[b] + t) % Tcap and no row is dropped (T <= Tcap on
// the host, so no slot is written twice).
// PAGED (both append kernels; the page rule: ops/decode.py): row p = lens[b] + t goes to page pt[b][p >> 8], row
// p & 255; kb, vb, ksb, vsb are the page strides. A position at or beyond Tcap, or whose table entry lies outside
// [0, n_pages), is dropped without a store.
// The kernels' names and parameter lists are those of the flat and ring forms as they were; the paged forms are
// kernels of their own: kv_append_paged over this body, kv_append_fp8_paged written out (the comment there).
template <bool RING, bool PAGED>
__device__ __forceinline__ void kv_append_rows(const __bf16* __restrict__ qkv, __bf16* __restrict__ kc,
                                               __bf16* __restrict__ vc, const int* __restrict__ pos, int B, int T,
                                               int H, int D8, int Tcap, long long qb, long long qt, long long kb,
                                               long long kh, long long kt, long long vb, long long vh, long long vt,
                                               int Hq,  // Hq q heads come before the H k heads
                                               const int* __restrict__ pt, long long pts, int n_pages) {
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
  long long row = (long long)pos[b] + t;
  if constexpr (RING) {
    if (row < 0) return;
    row = (unsigned)row % (unsigned)Tcap;  // below 2^32: an int32 length plus t
  } else {
    if (row < 0 || row >= Tcap) return;  // past the capacity: dropped, never written
  }
  int sl = b;  // the slice of the cache's first dimension
  if constexpr (PAGED) {
    sl = pt[b * pts + (row >> 8)];
    if (sl < 0 || sl >= n_pages) return;  // no page: dropped
    row &= 255;
  }
  const u32x4 val =
      *reinterpret_cast<const u32x4*>(qkv + b * qb + t * qt + ((long long)Hq + s * H + h) * (D8 * 8) + d8 * 8);
  __bf16* dst = s == 0 ? kc + sl * kb + h * kh + row * kt : vc + sl * vb + h * vh + row * vt;
  *reinterpret_cast<u32x4*>(dst + d8 * 8) = val;
}

template <bool RING>
__global__ __launch_bounds__(256) void kv_append(const __bf16* __restrict__ qkv, __bf16* __restrict__ kc,
                                                 __bf16* __restrict__ vc, const int* __restrict__ pos, int B, int T,
                                                 int H, int D8, int Tcap, long long qb, long long qt, long long kb,
                                                 long long kh, long long kt, long long vb, long long vh,
                                                 long long vt, int Hq) {
  kv_append_rows<RING, false>(qkv, kc, vc, pos, B, T, H, D8, Tcap, qb, qt, kb, kh, kt, vb, vh, vt, Hq, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void kv_append_paged(const __bf16* __restrict__ qkv, __bf16* __restrict__ kc,
                                                       __bf16* __restrict__ vc, const int* __restrict__ pos, int B,
                                                       int T, int H, int D8, int Tcap, long long qb, long long qt,
                                                       long long kb, long long kh, long long kt, long long vb,
                                                       long long vh, long long vt, int Hq,
                                                       const int* __restrict__ pt, long long pts, int n_pages) {
  kv_append_rows<false, true>(qkv, kc, vc, pos, B, T, H, D8, Tcap, qb, qt, kb, kh, kt, vb, vh, vt, Hq, pt, pts,
                              n_pages);
}

// One lane group (D / 8 lanes) per (b, t, k-or-v, h) row: a 16-B load of 8 bf16 per lane, the row's
// amax by the group reduction, one scale store by the group's first lane, one 8-B code store per lane.
// Groups are whole: the thread count is a multiple of D / 8 and so is the block size, and both early
// returns are group-uniform.
template <int D, bool RING>
__global__ __launch_bounds__(256) void kv_append_fp8(const __bf16* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                     uint8_t* __restrict__ vc, float* __restrict__ ks,
                                                     float* __restrict__ vs, const int* __restrict__ pos, int B, int T,
                                                     int H, int Tcap, long long qb, long long qt, long long kb,
                                                     long long kh, long long kt, long long vb, long long vh,
                                                     long long vt, long long ksb, long long ksh, long long vsb,
                                                     long long vsh, int Hq) {
  constexpr int G = D / 8;
  const long long n = (long long)B * T * 2 * H * G;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int piece = (int)(r % G);
  r /= G;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % 2);  // 0: k, 1: v
  r /= 2;
  const int t = (int)(r % T);
  const int b = (int)(r / T);
  long long row = (long long)pos[b] + t;
  if constexpr (RING) {
    if (row < 0) return;
    row = (unsigned)row % (unsigned)Tcap;
  } else {
    if (row < 0 || row >= Tcap) return;  // past the capacity: dropped, neither codes nor scale written
  }
  float x[8];
  Bf16Rows::unpack8(
      *reinterpret_cast<const u32x4*>(qkv + b * qb + t * qt + ((long long)Hq + s * H + h) * D + piece * 8), x);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
  am = kfw::group_max<G>(am);
  const float scale = am > 0.f ? am / kFp8Max : 1.f;  // IEEE division: the torch reference's scale
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] / scale, -kFp8Max), kFp8Max);
  u32x2 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i], y[4 * i + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i + 2], y[4 * i + 3], p, true);
    w[i] = (unsigned)p;
  }
  uint8_t* dst = s == 0 ? kc + b * kb + h * kh + row * kt : vc + b * vb + h * vh + row * vt;
  *reinterpret_cast<u32x2*>(dst + piece * 8) = w;
  if (piece == 0) {
    float* sd = s == 0 ? ks + b * ksb + h * ksh : vs + b * vsb + h * vsh;
    sd[row] = scale;
  }
}

// The paged form of kv_append_fp8 (the comment above kv_append): a kernel of its own with the same arithmetic, so that
// the flat and ring kernels stay instruction for instruction what they were (as one body inlined into both, the flat
// instantiations came out with two multiplications' operands swapped).
template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8_paged(const __bf16* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                     uint8_t* __restrict__ vc, float* __restrict__ ks,
                                                     float* __restrict__ vs, const int* __restrict__ pos, int B, int T,
                                                     int H, int Tcap, long long qb, long long qt, long long kb,
                                                     long long kh, long long kt, long long vb, long long vh,
                                                     long long vt, long long ksb, long long ksh, long long vsb,
                                                     long long vsh, int Hq, const int* __restrict__ pt,
                                                     long long pts, int n_pages) {
  constexpr int G = D / 8;
  const long long n = (long long)B * T * 2 * H * G;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int piece = (int)(r % G);
  r /= G;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % 2);  // 0: k, 1: v
  r /= 2;
  const int t = (int)(r % T);
  const int b = (int)(r / T);
  long long row = (long long)pos[b] + t;
  if (row < 0 || row >= Tcap) return;  // past the capacity: dropped, neither codes nor scale written
  const int page = pt[b * pts + (row >> 8)];  // uniform over the row's lane group
  if (page < 0 || page >= n_pages) return;    // no page: dropped
  row &= 255;
  float x[8];
  Bf16Rows::unpack8(
      *reinterpret_cast<const u32x4*>(qkv + b * qb + t * qt + ((long long)Hq + s * H + h) * D + piece * 8), x);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
  am = kfw::group_max<G>(am);
  const float scale = am > 0.f ? am / kFp8Max : 1.f;  // IEEE division: the torch reference's scale
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] / scale, -kFp8Max), kFp8Max);
  u32x2 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i], y[4 * i + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * i + 2], y[4 * i + 3], p, true);
    w[i] = (unsigned)p;
  }
  uint8_t* dst = s == 0 ? kc + page * kb + h * kh + row * kt : vc + page * vb + h * vh + row * vt;
  *reinterpret_cast<u32x2*>(dst + piece * 8) = w;
  if (piece == 0) {
    float* sd = s == 0 ? ks + page * ksb + h * ksh : vs + page * vsb + h * vsh;
    sd[row] = scale;
  }
}

}  // namespace

hipError_t kfkv::launch_kv_combine(int D, const float* ws, __bf16* o, float* lse, int B, int H, int Tq, int nsplit,
                                   long long ob, long long ot, long long oh, hipStream_t s, int lg) {
  const dim3 cgrid((unsigned)H, (unsigned)B, (unsigned)Tq);
  if (lg > 0 && D == 64)
    hipLaunchKernelGGL(attn_kv_combine_gqa<64>, cgrid, dim3(64), 0, s, ws, o, lse, B, H, Tq, nsplit, ob, ot, oh, lg);
  else if (lg > 0)
    hipLaunchKernelGGL(attn_kv_combine_gqa<128>, cgrid, dim3(128), 0, s, ws, o, lse, B, H, Tq, nsplit, ob, ot, oh, lg);
  else if (D == 64)
    hipLaunchKernelGGL(attn_kv_combine<64>, cgrid, dim3(64), 0, s, ws, o, lse, B, H, Tq, nsplit, ob, ot, oh);
  else
    hipLaunchKernelGGL(attn_kv_combine<128>, cgrid, dim3(128), 0, s, ws, o, lse, B, H, Tq, nsplit, ob, ot, oh);
  return hipGetLastError();
}

extern "C" int kfamd_attn_decode_split_keys(void) { return kSplitKeys; }

extern "C" long long kfamd_attn_decode_workspace(int B, int H, int D, int t_bound) {
  if (B <= 0 || H <= 0 || (D != 64 && D != 128) || t_bound < 1) return 0;
  const long long nsplit = (t_bound + kSplitKeys - 1) / kSplitKeys;
  return (long long)B * H * nsplit * (D + 2) * (long long)sizeof(float);
}

extern "C" long long kfamd_attn_extend_workspace(int B, int H, int D, int Tq, int t_bound) {
  if (Tq < 1 || Tq > kMaxRows) return 0;
  return kfamd_attn_decode_workspace(B, H, D, t_bound) * Tq;
}

// The four attention entry points (stride layouts: kfamd_kernels.h). Decode is Tq = 1 without t strides.
extern "C" int kfamd_attn_decode_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                      float* lse, void* ws, int B, int H, int D, int t_bound, float scale,
                                      const long long* st, void* stream) {
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                           false, stream);
}

extern "C" int kfamd_attn_extend_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                      float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
                                      const long long* st, void* stream) {
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, H, D, Tq, t_bound, scale, st,
                           true, stream);
}

extern "C" int kfamd_attn_decode_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                     const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                     int D, int t_bound, float scale, const long long* st, void* stream) {
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                          false, stream);
}

extern "C" int kfamd_attn_extend_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                     const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                     int D, int Tq, int t_bound, float scale, const long long* st, void* stream) {
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, H, D, Tq, t_bound, scale, st,
                          true, stream);
}

// The grouped-query forms (contract: kfamd_kernels.h): Hkv K / V heads, G query heads on each, T tokens:
// T * G <= 16 rows per (b, K / V head) on the extend kernels. Decode is T = 1 with t strides of 0.
extern "C" long long kfamd_attn_extend_gqa_workspace(int B, int Hkv, int G, int D, int T, int t_bound) {
  const int lg = group_log2(G);
  if (lg < 0 || T < 1 || T > (kMaxRows >> lg)) return 0;
  return kfamd_attn_decode_workspace(B, Hkv, D, t_bound) * (T << lg);
}

extern "C" int kfamd_attn_extend_gqa_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                          void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                          int t_bound, float scale, const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                           true, stream, G);
}

extern "C" int kfamd_attn_extend_gqa_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                         const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                         int Hkv, int G, int D, int T, int t_bound, float scale, const long long* st,
                                         void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                          true, stream, G);
}

// The sliding-window forms (contract: kfamd_kernels.h): the entry points above with a window of W >= 1 keys.
// Decode is the single-row kernel; extend takes the grouped signature, G = 1 for plain rows.
extern "C" int kfamd_attn_decode_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                          void* o, float* lse, void* ws, int B, int H, int D, int t_bound, int window,
                                          float scale, const long long* st, void* stream) {
  if (window < 1) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                           false, stream, 0, window);
}

extern "C" int kfamd_attn_decode_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                         const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                         int H, int D, int t_bound, int window, float scale, const long long* st,
                                         void* stream) {
  if (window < 1) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                          false, stream, 0, window);
}

extern "C" int kfamd_attn_extend_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                          void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                          int t_bound, int window, float scale, const long long* st, void* stream) {
  if (G <= 0 || window < 1) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                           true, stream, G, window);
}

extern "C" int kfamd_attn_extend_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                         const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                         int Hkv, int G, int D, int T, int t_bound, int window, float scale,
                                         const long long* st, void* stream) {
  if (G <= 0 || window < 1) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                          true, stream, G, window);
}

// K and V rows of a fused QKV activation [B][T][3][H][D] (element strides qb, qt; [3][H][D] dense)
// into the caches [B][H][Tcap][D] (strides b, h, t) at rows pos[b] .. pos[b] + T - 1. pos: device
// int32 [B], not advanced here. Rows at or beyond Tcap are dropped.
static int kv_append_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int Hq, int H,
                          int D, int Tcap, long long qb, long long qt, const long long* cache_strides, void* stream,
                          bool ring = false, const int* pt = nullptr, long long pts = 0, int n_pages = 0) {
  if (ring && (Tcap <= 0 || Tcap % kSplitKeys || T > Tcap)) return KFAMD_EINVAL;
  if (pt && (ring || n_pages < 1 || Tcap <= 0 || Tcap % kSplitKeys || pts < Tcap / kSplitKeys || !al4(pt)))
    return KFAMD_EINVAL;
  if (!qkv || !k_cache || !v_cache || !pos || !cache_strides || B <= 0 || T <= 0 || H <= 0 || D <= 0 || D % 8 ||
      Tcap <= 0 || Hq < H || Hq % H || group_log2(Hq / H) < 0)
    return KFAMD_EINVAL;
  const long long* c = cache_strides;
  if (!al16(qkv) || !al16(k_cache) || !al16(v_cache)) return KFAMD_EALIGN;
  if ((qb | qt | c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & 7) return KFAMD_EALIGN;
  const long long n = (long long)B * T * 2 * H * (D / 8);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (pt)
    hipLaunchKernelGGL(kv_append_paged, grid, dim3(256), 0, s, static_cast<const __bf16*>(qkv),
                       static_cast<__bf16*>(k_cache), static_cast<__bf16*>(v_cache), pos, B, T, H, D / 8, Tcap, qb, qt,
                       c[0], c[1], c[2], c[3], c[4], c[5], Hq, pt, pts, n_pages);
  else if (ring)
    hipLaunchKernelGGL(kv_append<true>, grid, dim3(256), 0, s, static_cast<const __bf16*>(qkv),
                       static_cast<__bf16*>(k_cache), static_cast<__bf16*>(v_cache), pos, B, T, H, D / 8, Tcap, qb, qt,
                       c[0], c[1], c[2], c[3], c[4], c[5], Hq);
  else
    hipLaunchKernelGGL(kv_append<false>, grid, dim3(256), 0, s, static_cast<const __bf16*>(qkv),
                       static_cast<__bf16*>(k_cache), static_cast<__bf16*>(v_cache), pos, B, T, H, D / 8, Tcap, qb, qt,
                       c[0], c[1], c[2], c[3], c[4], c[5], Hq);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

extern "C" int kfamd_kv_append_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int H,
                                    int D, int Tcap, long long qb, long long qt, const long long* cache_strides,
                                    void* stream) {
  return kv_append_bf16(qkv, k_cache, v_cache, pos, B, T, H, H, D, Tcap, qb, qt, cache_strides, stream);
}

// The same for a grouped-query layer: the activation is [B][T][(Hq + 2 Hkv) D], q: Hq D | k: Hkv D | v: Hkv D,
// the caches hold the Hkv heads. Hq / Hkv in {1, 2, 4, 8, 16}, KFAMD_EINVAL otherwise.
extern "C" int kfamd_kv_append_gqa_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T,
                                        int Hq, int Hkv, int D, int Tcap, long long qb, long long qt,
                                        const long long* cache_strides, void* stream) {
  if (Hkv <= 0) return KFAMD_EINVAL;
  return kv_append_bf16(qkv, k_cache, v_cache, pos, B, T, Hq, Hkv, D, Tcap, qb, qt, cache_strides, stream);
}

// The same rows quantised row by row into codes [B][H][Tcap][D] and scales [B][H][Tcap].
// cache_strides = {kb, kh, kt, vb, vh, vt, ksb, ksh, vsb, vsh}.
static int kv_append_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale, const int* pos,
                         int B, int T, int Hq, int H, int D, int Tcap, long long qb, long long qt,
                         const long long* cache_strides, void* stream, bool ring = false, const int* pt = nullptr,
                         long long pts = 0, int n_pages = 0) {
  if (ring && (Tcap <= 0 || Tcap % kSplitKeys || T > Tcap)) return KFAMD_EINVAL;
  if (pt && (ring || n_pages < 1 || Tcap <= 0 || Tcap % kSplitKeys || pts < Tcap / kSplitKeys || !al4(pt)))
    return KFAMD_EINVAL;
  if (!qkv || !k_codes || !v_codes || !k_scale || !v_scale || !pos || !cache_strides || B <= 0 || T <= 0 || H <= 0 ||
      Tcap <= 0 || Hq < H || Hq % H || group_log2(Hq / H) < 0)
    return KFAMD_EINVAL;
  if (D != 64 && D != 128) return KFAMD_EINVAL;
  const long long* c = cache_strides;
  if (c[2] < D || c[5] < D) return KFAMD_EINVAL;
  if (!al16(qkv) || !al16(k_codes) || !al16(v_codes) || !al4(k_scale) || !al4(v_scale)) return KFAMD_EALIGN;
  if ((qb | qt) & 7) return KFAMD_EALIGN;
  if ((c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & 15) return KFAMD_EALIGN;
  const long long n = (long long)B * T * 2 * H * (D / 8);
  if ((n + 255) / 256 > 0x7fffffffll) return KFAMD_EINVAL;
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const __bf16* x = static_cast<const __bf16*>(qkv);
  uint8_t* kc = static_cast<uint8_t*>(k_codes);
  uint8_t* vc = static_cast<uint8_t*>(v_codes);
#define KF_APPEND_FP8(DD, RR)                                                                                         \
  hipLaunchKernelGGL((kv_append_fp8<DD, RR>), grid, dim3(256), 0, s, x, kc, vc, k_scale, v_scale, pos, B, T, H, Tcap, \
                     qb, qt, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], Hq)
#define KF_APPEND_FP8_PAGED(DD)                                                                                      \
  hipLaunchKernelGGL((kv_append_fp8_paged<DD>), grid, dim3(256), 0, s, x, kc, vc, k_scale, v_scale, pos, B, T, H, Tcap, \
                     qb, qt, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], Hq, pt, pts, n_pages)
  if (D == 64 && pt) KF_APPEND_FP8_PAGED(64);
  else if (pt) KF_APPEND_FP8_PAGED(128);
  else if (D == 64 && ring) KF_APPEND_FP8(64, true);
  else if (D == 64) KF_APPEND_FP8(64, false);
  else if (ring) KF_APPEND_FP8(128, true);
  else KF_APPEND_FP8(128, false);
#undef KF_APPEND_FP8_PAGED
#undef KF_APPEND_FP8
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KFAMD_OK : static_cast<int>(e);
}

extern "C" int kfamd_kv_append_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                   const int* pos, int B, int T, int H, int D, int Tcap, long long qb, long long qt,
                                   const long long* cache_strides, void* stream) {
  return kv_append_fp8(qkv, k_codes, v_codes, k_scale, v_scale, pos, B, T, H, H, D, Tcap, qb, qt, cache_strides,
                       stream);
}

extern "C" int kfamd_kv_append_gqa_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                       const int* pos, int B, int T, int Hq, int Hkv, int D, int Tcap, long long qb,
                                       long long qt, const long long* cache_strides, void* stream) {
  if (Hkv <= 0) return KFAMD_EINVAL;
  return kv_append_fp8(qkv, k_codes, v_codes, k_scale, v_scale, pos, B, T, Hq, Hkv, D, Tcap, qb, qt, cache_strides,
                       stream);
}

// The ring forms (contract: kfamd_kernels.h; the rule: the docstring of ops/decode.py). The attention entry points take
// the windowed signatures with the ring's capacity C in t_bound's place; the appends the grouped signatures.
extern "C" int kfamd_attn_ring_nsplit(int window, int T) {
  return window >= 1 && T >= 1 ? ring_splits(window, T) : 0;
}

extern "C" long long kfamd_attn_decode_ring_workspace(int B, int H, int D, int window) {
  if (window < 1) return 0;
  return kfamd_attn_decode_workspace(B, H, D, ring_splits(window, 1) * kSplitKeys);
}

extern "C" long long kfamd_attn_extend_ring_workspace(int B, int Hkv, int G, int D, int T, int window) {
  if (window < 1 || T < 1) return 0;
  return kfamd_attn_extend_gqa_workspace(B, Hkv, G, D, T, ring_splits(window, T) * kSplitKeys);
}

extern "C" int kfamd_attn_decode_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                           void* o, float* lse, void* ws, int B, int H, int D, int cap, int window,
                                           float scale, const long long* st, void* stream) {
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, H, D, 1, cap, scale, st, false,
                           stream, 0, window, true);
}

extern "C" int kfamd_attn_decode_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                          const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                          int H, int D, int cap, int window, float scale, const long long* st,
                                          void* stream) {
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, H, D, 1, cap, scale, st, false,
                          stream, 0, window, true);
}

extern "C" int kfamd_attn_extend_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens,
                                           void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T, int cap,
                                           int window, float scale, const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_cache, v_cache, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, cap, scale, st, true,
                           stream, G, window, true);
}

extern "C" int kfamd_attn_extend_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                                          const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B,
                                          int Hkv, int G, int D, int T, int cap, int window, float scale,
                                          const long long* st, void* stream) {
  if (G <= 0) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_codes, v_codes, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, cap, scale, st, true,
                          stream, G, window, true);
}

extern "C" int kfamd_kv_append_ring_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T,
                                         int Hq, int Hkv, int D, int cap, long long qb, long long qt,
                                         const long long* cache_strides, void* stream) {
  if (Hkv <= 0) return KFAMD_EINVAL;
  return kv_append_bf16(qkv, k_cache, v_cache, pos, B, T, Hq, Hkv, D, cap, qb, qt, cache_strides, stream, true);
}

extern "C" int kfamd_kv_append_ring_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                        const int* pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb,
                                        long long qt, const long long* cache_strides, void* stream) {
  if (Hkv <= 0) return KFAMD_EINVAL;
  return kv_append_fp8(qkv, k_codes, v_codes, k_scale, v_scale, pos, B, T, Hq, Hkv, D, cap, qb, qt, cache_strides,
                       stream, true);
}

// The paged forms (contract: kfamd_kernels.h; the page rule: the docstring of ops/decode.py). The attention entry
// points take decode's / the grouped signatures, the appends the grouped ones, each with the page table before the
// stream; the b entries of the stride arrays are the page strides.
extern "C" int kfamd_attn_decode_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens,
                                            void* o, float* lse, void* ws, int B, int H, int D, int t_bound,
                                            float scale, const long long* st, const int* page_table,
                                            long long table_stride, int n_pages, void* stream) {
  if (!page_table) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_pages, v_pages, nullptr, nullptr, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                           false, stream, 0, 0, false, page_table, table_stride, n_pages);
}

extern "C" int kfamd_attn_decode_paged_fp8(const void* q, const void* k_pages, const void* v_pages,
                                           const float* k_scale, const float* v_scale, const int* lens, void* o,
                                           float* lse, void* ws, int B, int H, int D, int t_bound, float scale,
                                           const long long* st, const int* page_table, long long table_stride,
                                           int n_pages, void* stream) {
  if (!page_table) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_pages, v_pages, k_scale, v_scale, lens, o, lse, ws, B, H, D, 1, t_bound, scale, st,
                          false, stream, 0, 0, false, page_table, table_stride, n_pages);
}

extern "C" int kfamd_attn_extend_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens,
                                            void* o, float* lse, void* ws, int B, int Hkv, int G, int D, int T,
                                            int t_bound, float scale, const long long* st, const int* page_table,
                                            long long table_stride, int n_pages, void* stream) {
  if (G <= 0 || !page_table) return KFAMD_EINVAL;
  return attn_kv<Bf16Rows>(q, k_pages, v_pages, nullptr, nullptr, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                           true, stream, G, 0, false, page_table, table_stride, n_pages);
}

extern "C" int kfamd_attn_extend_paged_fp8(const void* q, const void* k_pages, const void* v_pages,
                                           const float* k_scale, const float* v_scale, const int* lens, void* o,
                                           float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound,
                                           float scale, const long long* st, const int* page_table,
                                           long long table_stride, int n_pages, void* stream) {
  if (G <= 0 || !page_table) return KFAMD_EINVAL;
  return attn_kv<Fp8Rows>(q, k_pages, v_pages, k_scale, v_scale, lens, o, lse, ws, B, Hkv, D, T, t_bound, scale, st,
                          true, stream, G, 0, false, page_table, table_stride, n_pages);
}

extern "C" int kfamd_kv_append_paged_bf16(const void* qkv, void* k_pages, void* v_pages, const int* pos, int B, int T,
                                          int Hq, int Hkv, int D, int cap, long long qb, long long qt,
                                          const long long* cache_strides, const int* page_table,
                                          long long table_stride, int n_pages, void* stream) {
  if (Hkv <= 0 || !page_table) return KFAMD_EINVAL;
  return kv_append_bf16(qkv, k_pages, v_pages, pos, B, T, Hq, Hkv, D, cap, qb, qt, cache_strides, stream, false,
                        page_table, table_stride, n_pages);
}

extern "C" int kfamd_kv_append_paged_fp8(const void* qkv, void* k_pages, void* v_pages, float* k_scale, float* v_scale,
                                         const int* pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb,
                                         long long qt, const long long* cache_strides, const int* page_table,
                                         long long table_stride, int n_pages, void* stream) {
  if (Hkv <= 0 || !page_table) return KFAMD_EINVAL;
  return kv_append_fp8(qkv, k_pages, v_pages, k_scale, v_scale, pos, B, T, Hq, Hkv, D, cap, qb, qt, cache_strides,
                       stream, false, page_table, table_stride, n_pages);
}
